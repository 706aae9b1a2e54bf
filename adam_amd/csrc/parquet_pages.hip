// Parquet data page bodies built on the device (include/adam_sam.h:
// bqsr_parquet_pages_*): the definition levels and the values of one column
// chunk, cut into V1 data pages of page_rows rows, from columns that already
// lie in device memory.  The page forms: definition levels (max level 1) as
// the validity bitmap in one bit-packed run, PLAIN int32 / int64 with the
// nulls compacted out, dictionary indices in the RLE / bit-packed hybrid
// under the header's block rule, and -- from Arrow string and boolean columns
// (bqsr_parquet_pages_size_strings / _bools) -- PLAIN BYTE_ARRAY and PLAIN
// BOOLEAN.  Page headers, dictionary pages, the codec and the footer are the
// host's (adam_amd/parquet_pages.py).
//
// A column chunk is a sequence of ITEMS, 1 + page_rows / 64 per page: item 0
// of a page is its preamble (the levels, and a dictionary page's bit-width
// byte), item k >= 1 the k-th block of 64 of the page's non-null values.  A
// wavefront takes an item, so no lane ever walks a page:
//
//   pq_levels   a wavefront per 64-row word: every lane evaluates its row
//               (validity bit, gather, remap, base), one ballot is the word of
//               the page's levels and its popcount the word's non-nulls.
//   (scan)      the words' non-null counts: every word's first value.
//   pq_compact  the same evaluation, each non-null lane storing its value at
//               the word's first value + the ballot's prefix popcount: a
//               wavefront stores contiguous values.
//   pq_items    a wavefront per item: its size in bytes -- for a block of
//               indices one wave-wide compare decides between an RLE run of 64
//               and a bit-packed run.
//   (scan)      the items' sizes: every item's offset, and the chunk's size
//               before any output memory is taken.
//   pq_emit     a wavefront per item writes its bytes.  A lane owns whole
//               output bytes (the preamble and the packed indices: a byte per
//               lane and step; PLAIN values: a value per lane), so no two
//               lanes touch one byte and every store is a vector store.
//
// The string and boolean forms go the same way with kernels of their own:
// pq_bitmap_levels (the validity words are the level words), pq_compact_bytes
// (strings: the non-null rows' INDICES are what is compacted; booleans: a byte
// per non-null bit), pq_items_bytes (a block of strings is the wave sum of
// 4 + length, a block of n bits ceil(n / 8) bytes) and
// pq_emit_bytes: the wavefront prefix-sums its 64 sizes, every lane stores its
// length word, then the 64 strings are copied one after another, a byte per
// lane and step (adlk::wave_copy, as adam_lines_write does); of a block of bits
// one ballot is the 8 bytes, a byte per lane.
//
// Included by bqsr_capi.cpp after pileup.hip.

namespace pqk {

constexpr int kThreads = 256;

__device__ __forceinline__ int varint_len(uint32_t v) {
  int n = 1;
  while (v >= 128u) {
    v >>= 7;
    ++n;
  }
  return n;
}
__device__ __forceinline__ uint8_t varint_byte(uint32_t v, int k, int len) {
  return (uint8_t)(((v >> (7 * k)) & 0x7Fu) | (k + 1 < len ? 0x80u : 0u));
}

// row g of the column: false when null, else the value (index columns: after remap and base)
__device__ __forceinline__ bool row_value(const bqsr_parquet_column& c, int64_t g, int64_t* out) {
  if (c.validity && !((c.validity[g >> 6] >> (g & 63)) & 1ull)) return false;
  const int64_t i = c.gather ? (int64_t)c.gather[g] : g;
  if (i < 0 || i >= c.src_n) return false;
  int64_t v = c.src_width == 1   ? (int64_t)((const uint8_t*)c.src)[i]
              : c.src_width == 4 ? (int64_t)((const int32_t*)c.src)[i]
                                 : ((const int64_t*)c.src)[i];
  if (c.remap) {
    if (v < 0 || v >= (int64_t)c.remap_n) return false;
    v = c.remap[v];
    if (v < 0) return false;
  }
  *out = v - c.base;
  return true;
}

// how a chunk is cut
struct Geo {
  int64_t n_rows, n_words, n_pages, n_items;
  int32_t page_words;  // page_rows / 64
  int32_t per_page;    // items per page: 1 + page_words
  int32_t kind;
  int32_t value_bytes;  // of a compacted value: 8 for PLAIN int64, else 4
  int32_t bit_width;
};

__device__ __forceinline__ int64_t wave_index() { return (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; }
__device__ __forceinline__ int64_t wave_count() { return ((int64_t)gridDim.x * blockDim.x) >> 6; }

extern "C" __global__ void __launch_bounds__(kThreads) pq_levels(bqsr_parquet_column c, Geo G, uint64_t* vword,
                                                                 uint64_t* cnt) {
  const int lane = threadIdx.x & 63;
  for (int64_t w = wave_index(); w < G.n_words; w += wave_count()) {
    const int64_t g = (w << 6) + lane;
    int64_t v;
    const bool has = g < G.n_rows && row_value(c, g, &v);
    const uint64_t b = __builtin_amdgcn_ballot_w64(has);
    if (lane == 0) {
      vword[w] = b;
      cnt[w] = (uint64_t)__popcll(b);
    }
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) pq_compact(bqsr_parquet_column c, Geo G, const uint64_t* vword,
                                                                  const uint64_t* voff, void* vals) {
  const int lane = threadIdx.x & 63;
  const uint64_t mask = G.bit_width >= 32 ? 0xFFFFFFFFull : ((1ull << G.bit_width) - 1ull);
  for (int64_t w = wave_index(); w < G.n_words; w += wave_count()) {
    const uint64_t b = vword[w];
    if (!((b >> lane) & 1ull)) continue;
    int64_t v = 0;
    (void)row_value(c, (w << 6) + lane, &v);
    const uint64_t at = voff[w] + (uint64_t)__popcll(b & ((1ull << lane) - 1ull));
    if (G.value_bytes == 8) ((int64_t*)vals)[at] = v;
    else if (G.kind == BQSR_PARQUET_DICT_INDEX) ((uint32_t*)vals)[at] = (uint32_t)((uint64_t)v & mask);
    else ((uint32_t*)vals)[at] = (uint32_t)v;
  }
}

// what an item's wavefront knows of its page
struct PageOf {
  int64_t page, w0, rows, first, non_nulls;  // first: the page's first compacted value
  int32_t k;                                 // the item within the page
};
__device__ __forceinline__ PageOf page_of(const Geo& G, const uint64_t* voff, int64_t item) {
  PageOf P;
  P.page = item / G.per_page;
  P.k = (int32_t)(item - P.page * G.per_page);
  P.w0 = P.page * G.page_words;
  const int64_t w1 = min(G.n_words, P.w0 + G.page_words);
  P.rows = min((int64_t)G.page_words << 6, G.n_rows - (P.w0 << 6));
  P.first = (int64_t)voff[P.w0];
  P.non_nulls = (int64_t)voff[w1] - P.first;
  return P;
}
// the preamble: u32 length of the levels, the bit-packed run's header, the bitmap bytes
__device__ __forceinline__ uint32_t level_header(int64_t rows) { return ((uint32_t)((rows + 7) >> 3) << 1) | 1u; }

// the block of 64 at `at`: whether it is an RLE run (full, every value equal)
__device__ __forceinline__ bool equal_block(const uint32_t* vals, int64_t at, int64_t n, int lane, uint32_t* mine) {
  const uint32_t v = lane < n ? vals[at + lane] : 0u;
  *mine = v;
  const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
  return n == 64 && __builtin_amdgcn_ballot_w64(v == first) == ~0ull;
}

extern "C" __global__ void __launch_bounds__(kThreads) pq_items(Geo G, const uint64_t* voff, const void* vals,
                                                                uint64_t* size) {
  const int lane = threadIdx.x & 63;
  for (int64_t item = wave_index(); item < G.n_items; item += wave_count()) {
    const PageOf P = page_of(G, voff, item);
    uint64_t bytes = 0;
    if (P.k == 0) {
      const int64_t nb = (P.rows + 7) >> 3;
      bytes = (uint64_t)(4 + varint_len(level_header(P.rows)) + nb + (G.kind == BQSR_PARQUET_DICT_INDEX ? 1 : 0));
    } else {
      const int64_t b0 = (int64_t)(P.k - 1) << 6;
      const int64_t n = min((int64_t)64, P.non_nulls - b0);
      if (n > 0) {
        if (G.kind != BQSR_PARQUET_DICT_INDEX) {
          bytes = (uint64_t)n * (uint64_t)G.value_bytes;
        } else {
          uint32_t v;
          const bool rle = equal_block((const uint32_t*)vals, P.first + b0, n, lane, &v);
          bytes = rle ? (uint64_t)(2 + ((G.bit_width + 7) >> 3)) : (uint64_t)(1 + ((n + 7) >> 3) * G.bit_width);
        }
      }
    }
    if (lane == 0) size[item] = bytes;
  }
}

template <class T>
__device__ __forceinline__ void store_bytes(uint8_t* at, T v) {
  __builtin_memcpy(at, &v, sizeof(T));  // (a page body starts at any byte)
}

// item 0 of a page: the preamble's bytes (a byte per lane and step), a dictionary page's bit-width byte and the
// page's entry of the page table
__device__ __forceinline__ void emit_preamble(const Geo& G, const PageOf& P, const uint64_t* vword,
                                              const uint64_t* ioff, int64_t item, uint8_t* o, bqsr_parquet_page* pages,
                                              int lane) {
  const int64_t nb = (P.rows + 7) >> 3;
  const uint32_t head = level_header(P.rows);
  const int vl = varint_len(head);
  const uint32_t len = (uint32_t)(vl + nb);
  const int64_t pre = 4 + vl + nb;
  for (int64_t t = lane; t < pre; t += 64) {
    uint8_t x;
    if (t < 4) x = (uint8_t)(len >> (8 * t));
    else if (t < 4 + vl) x = varint_byte(head, (int)(t - 4), vl);
    else {
      const int64_t kb = t - 4 - vl;
      x = (uint8_t)(vword[P.w0 + (kb >> 3)] >> (8 * (kb & 7)));
    }
    o[t] = x;
  }
  if (lane == 0) {
    if (G.kind == BQSR_PARQUET_DICT_INDEX) o[pre] = (uint8_t)G.bit_width;
    const int64_t a = (int64_t)ioff[item], b = (int64_t)ioff[item + G.per_page];
    pages[P.page] = bqsr_parquet_page{a, b - a, P.rows, P.non_nulls};
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) pq_emit(Geo G, const uint64_t* vword, const uint64_t* voff,
                                                               const void* vals, const uint64_t* ioff, uint8_t* out,
                                                               bqsr_parquet_page* pages) {
  const int lane = threadIdx.x & 63;
  for (int64_t item = wave_index(); item < G.n_items; item += wave_count()) {
    const PageOf P = page_of(G, voff, item);
    uint8_t* o = out + ioff[item];
    if (P.k == 0) {
      emit_preamble(G, P, vword, ioff, item, o, pages, lane);
      continue;
    }
    const int64_t b0 = (int64_t)(P.k - 1) << 6;
    const int64_t n = min((int64_t)64, P.non_nulls - b0);
    if (n <= 0) continue;
    const int64_t at = P.first + b0;
    if (G.kind != BQSR_PARQUET_DICT_INDEX) {
      if (lane < n) {
        if (G.value_bytes == 8) store_bytes(o + 8 * lane, ((const int64_t*)vals)[at + lane]);
        else store_bytes(o + 4 * lane, ((const uint32_t*)vals)[at + lane]);
      }
      continue;
    }
    const uint32_t* idx = (const uint32_t*)vals;
    const int w = G.bit_width;
    uint32_t v;
    if (equal_block(idx, at, n, lane, &v)) {  // <varint 64 << 1> <the value in ceil(w / 8) bytes>
      const int vb = (w + 7) >> 3;
      if (lane == 0) o[0] = 0x80;
      else if (lane == 1) o[1] = 0x01;
      else if (lane < 2 + vb) o[lane] = (uint8_t)(v >> (8 * (lane - 2)));
      continue;
    }
    // <varint groups << 1 | 1> <groups * 8 values of w bits, LSB first, the tail zero-padded>
    const int groups = (int)((n + 7) >> 3);
    if (lane == 0) o[0] = (uint8_t)((groups << 1) | 1);
    const int total = groups * w;  // bytes
    for (int t = lane; t < total; t += 64) {
      const int bit0 = 8 * t;
      uint64_t acc = 0;
      for (int q = bit0 / w; q * w < bit0 + 8 && q < n; ++q) {
        const uint64_t x = idx[at + q];
        const int sh = q * w - bit0;
        acc |= sh >= 0 ? (x << sh) : (x >> -sh);
      }
      o[1 + t] = (uint8_t)acc;
    }
  }
}

// ---- PLAIN BYTE_ARRAY from an Arrow string column, PLAIN BOOLEAN from an Arrow bitmap ----

// the validity words are the level words (none: every row present), the bits beyond n_rows cleared
extern "C" __global__ void __launch_bounds__(kThreads) pq_bitmap_levels(const uint64_t* validity, Geo G,
                                                                        uint64_t* vword, uint64_t* cnt) {
  for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < G.n_words; w += (int64_t)gridDim.x * blockDim.x) {
    uint64_t b = validity ? validity[w] : ~0ull;
    const int64_t rest = G.n_rows - (w << 6);
    if (rest < 64) b &= (1ull << rest) - 1ull;
    vword[w] = b;
    cnt[w] = (uint64_t)__popcll(b);
  }
}

// what pq_compact does for values: strings, the non-null rows' indices (int32); booleans, a byte per non-null bit
extern "C" __global__ void __launch_bounds__(kThreads) pq_compact_bytes(Geo G, const uint64_t* vword,
                                                                        const uint64_t* voff, const uint64_t* bits,
                                                                        void* vals) {
  const int lane = threadIdx.x & 63;
  for (int64_t w = wave_index(); w < G.n_words; w += wave_count()) {
    const uint64_t b = vword[w];
    if (!((b >> lane) & 1ull)) continue;
    const uint64_t at = voff[w] + (uint64_t)__popcll(b & ((1ull << lane) - 1ull));
    if (G.kind == BQSR_PARQUET_PLAIN_BYTE_ARRAY) ((int32_t*)vals)[at] = (int32_t)((w << 6) + lane);
    else ((uint8_t*)vals)[at] = (uint8_t)((bits[w] >> lane) & 1ull);
  }
}

// lane's string of the block at `at` (n of them): where its bytes start and how many (a lane beyond n: none)
__device__ __forceinline__ int32_t block_string(const int32_t* rows, const int32_t* soff, int64_t at, int64_t n,
                                                int lane, int32_t* a) {
  *a = 0;
  if (lane >= n) return -1;
  const int32_t r = rows[at + lane];
  *a = soff[r];
  return max(0, soff[r + 1] - *a);
}

extern "C" __global__ void __launch_bounds__(kThreads) pq_items_bytes(Geo G, const uint64_t* voff, const void* vals,
                                                                      const int32_t* soff, uint64_t* size) {
  const int lane = threadIdx.x & 63;
  for (int64_t item = wave_index(); item < G.n_items; item += wave_count()) {
    const PageOf P = page_of(G, voff, item);
    uint64_t bytes = 0;
    if (P.k == 0) {
      bytes = (uint64_t)(4 + varint_len(level_header(P.rows)) + ((P.rows + 7) >> 3));
    } else {
      const int64_t b0 = (int64_t)(P.k - 1) << 6;
      const int64_t n = min((int64_t)64, P.non_nulls - b0);
      if (n > 0 && G.kind == BQSR_PARQUET_PLAIN_BOOLEAN) {
        bytes = (uint64_t)((n + 7) >> 3);
      } else if (n > 0) {  // the wave sum of 4 + length
        int32_t a;
        const int32_t len = block_string((const int32_t*)vals, soff, P.first + b0, n, lane, &a);
        bytes = len < 0 ? 0ull : 4ull + (uint64_t)len;
        for (int d = 32; d > 0; d >>= 1) bytes += (uint64_t)__shfl_xor((unsigned long long)bytes, d, 64);
      }
    }
    if (lane == 0) size[item] = bytes;
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) pq_emit_bytes(Geo G, const uint64_t* vword,
                                                                     const uint64_t* voff, const void* vals,
                                                                     const int32_t* soff, const uint8_t* sbytes,
                                                                     const uint64_t* ioff, uint8_t* out,
                                                                     bqsr_parquet_page* pages) {
  const int lane = threadIdx.x & 63;
  for (int64_t item = wave_index(); item < G.n_items; item += wave_count()) {
    const PageOf P = page_of(G, voff, item);
    uint8_t* o = out + ioff[item];
    if (P.k == 0) {
      emit_preamble(G, P, vword, ioff, item, o, pages, lane);
      continue;
    }
    const int64_t b0 = (int64_t)(P.k - 1) << 6;
    const int64_t n = min((int64_t)64, P.non_nulls - b0);  // (the same in every lane)
    if (n <= 0) continue;
    const int64_t at = P.first + b0;
    if (G.kind == BQSR_PARQUET_PLAIN_BOOLEAN) {  // one ballot is the block's 8 bytes, the bits past n clear
      const uint64_t word = __builtin_amdgcn_ballot_w64(lane < n && ((const uint8_t*)vals)[at + lane] != 0);
      if (lane < ((n + 7) >> 3)) o[lane] = (uint8_t)(word >> (8 * lane));
      continue;
    }
    // every lane's string starts at the prefix sum of the 4 + length before it: its length word by the lane,
    // then the strings' bytes by the whole wavefront, one string after another
    int32_t a;
    const int32_t len = block_string((const int32_t*)vals, soff, at, n, lane, &a);
    const uint32_t mine = len < 0 ? 0u : 4u + (uint32_t)len;  // (a column's bytes stay below 2^31)
    uint32_t upto = mine;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)upto, d, 64);
      if (lane >= d) upto += t;
    }
    const int64_t start = (int64_t)(upto - mine);
    if (len >= 0) store_bytes(o + start, (uint32_t)len);
    adlk::wave_copy(__builtin_amdgcn_ballot_w64(len > 0), sbytes, a, max(len, 0), o, start + 4, lane);
  }
}

// min, max and count of the column's non-null values: mm[0] min, mm[1] max, mm[2] count
extern "C" __global__ void __launch_bounds__(kThreads) pq_minmax(bqsr_parquet_column c, int64_t n_rows,
                                                                 long long* mm) {
  long long lo = INT64_MAX, hi = INT64_MIN, cnt = 0;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < n_rows; g += (int64_t)gridDim.x * blockDim.x) {
    int64_t v;
    if (row_value(c, g, &v)) {
      lo = min(lo, (long long)v);
      hi = max(hi, (long long)v);
      ++cnt;
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    lo = min(lo, __shfl_xor(lo, d, 64));
    hi = max(hi, __shfl_xor(hi, d, 64));
    cnt += __shfl_xor(cnt, d, 64);
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicMin(mm, lo);
    atomicMax(mm + 1, hi);
    atomicAdd((unsigned long long*)(mm + 2), (unsigned long long)cnt);
  }
}

}  // namespace pqk

struct bqsr_parquet_pages {
  bqsr_context* ctx = nullptr;
  DevBuf vword, cnt, voff, vals, isz, ioff, part, ptab, out, mm;
  pqk::Geo G{};
  int64_t body_bytes = 0;
  bool sized = false;
  // of the last bqsr_parquet_pages_size_strings: the column's offsets and bytes (the emit pass reads them again)
  const int32_t* s_off = nullptr;
  const uint8_t* s_bytes = nullptr;
  StageClock<4> clock;
  // of the last bqsr_parquet_pages_compress (snappy_pages.hip): the page table and the compressed pages' offsets
  // on the host, until the fetch; the codec's device scratch
  bool compressed = false;
  std::vector<bqsr_parquet_page> h_pages;
  std::vector<int64_t> comp_off;
  std::shared_ptr<void> codec;
};

namespace {

enum { PQ_SIZE, PQ_EMIT, PQ_STAGES };
enum { PQ_SIZE_0, PQ_SIZE_1, PQ_EMIT_0, PQ_EMIT_1 };
thread_local double g_pq_ms[PQ_STAGES] = {0.0, 0.0};
const char* kPqJob = "parquet pages";

bqsr_status pq_check(const bqsr_parquet_column* c, int64_t n_rows, const char* who) {
  const std::string w(who);
  if (!c || n_rows < 0 || n_rows > (int64_t)INT32_MAX) return fail(BQSR_ERR_INVALID_ARG, w + ": bad arguments");
  if (c->kind != BQSR_PARQUET_PLAIN_INT32 && c->kind != BQSR_PARQUET_PLAIN_INT64 && c->kind != BQSR_PARQUET_DICT_INDEX)
    return fail(BQSR_ERR_INVALID_ARG, w + ": unknown column kind");
  const bool w_ok = c->src_width == 1 || c->src_width == 4 || (c->src_width == 8 && c->kind == BQSR_PARQUET_PLAIN_INT64);
  if (!w_ok) return fail(BQSR_ERR_INVALID_ARG, w + ": source width must be 1 or 4 (8 for PLAIN int64)");
  if (c->kind == BQSR_PARQUET_DICT_INDEX && (c->bit_width < 1 || c->bit_width > 32))
    return fail(BQSR_ERR_INVALID_ARG, w + ": an index column's bit width is 1 to 32");
  if (c->kind != BQSR_PARQUET_DICT_INDEX && (c->remap || c->base))
    return fail(BQSR_ERR_INVALID_ARG, w + ": remap and base belong to index columns");
  if (c->remap && c->remap_n <= 0) return fail(BQSR_ERR_INVALID_ARG, w + ": a remap table without entries");
  if (n_rows && (!c->src || c->src_n < (c->gather ? 1 : n_rows)))
    return fail(BQSR_ERR_INVALID_ARG, w + ": the source does not cover the rows");
  return BQSR_OK;
}

unsigned pq_grid(const bqsr_context* ctx, int64_t waves) {
  return sam_grid(waves, pqk::kThreads / 64, ctx->tune_pileup_grid > 0 ? ctx->tune_pileup_grid : ctx->n_cu * 8);
}

// A size call's frame.  pq_begin: the refusals every size call shares, the chunk's geometry, and (rows at all:
// *live) the scratch and the stage's first mark; pq_finish: the items' offsets and the chunk's size.
struct PqScratch {
  uint64_t *vword, *cnt, *voff, *isz, *ioff, *part;
  uint8_t* vals;
};
bqsr_status pq_begin(bqsr_parquet_pages* enc, int64_t n_rows, int64_t page_rows, int32_t kind, int32_t value_bytes,
                     int32_t bit_width, hipStream_t s, bqsr_parquet_pages_sizes* out, const char* who, PqScratch* B,
                     bool* live) {
  *live = false;
  if (!enc || !out || page_rows <= 0 || page_rows % 64 || page_rows > (1 << 24))
    return fail(BQSR_ERR_INVALID_ARG, std::string(who) + ": bad arguments (page_rows is a multiple of 64)");
  if (n_rows < 0 || n_rows > (int64_t)INT32_MAX) return fail(BQSR_ERR_INVALID_ARG, std::string(who) + ": bad arguments");
  enc->sized = enc->compressed = false;
  g_pq_ms[PQ_SIZE] = g_pq_ms[PQ_EMIT] = 0.0;
  pqk::Geo& G = enc->G;
  G.n_rows = n_rows;
  G.n_words = (n_rows + 63) / 64;
  G.n_pages = (n_rows + page_rows - 1) / page_rows;
  G.page_words = (int32_t)(page_rows / 64);
  G.per_page = 1 + G.page_words;
  G.n_items = G.n_pages * G.per_page;
  G.kind = kind;
  G.value_bytes = value_bytes;
  G.bit_width = bit_width;
  enc->body_bytes = 0;
  out->n_pages = G.n_pages;
  out->body_bytes = 0;
  if (n_rows == 0) {
    enc->sized = true;
    return BQSR_OK;
  }
  HIP_TRY(hipSetDevice(enc->ctx->device));
  const size_t W = (size_t)G.n_words, I = (size_t)G.n_items;
  JOB_TRY(dev_need(enc->vword, &B->vword, W, kPqJob, "level words"));
  JOB_TRY(dev_need(enc->cnt, &B->cnt, W, kPqJob, "word counts"));
  JOB_TRY(dev_need(enc->voff, &B->voff, W + 1, kPqJob, "value offsets"));
  JOB_TRY(dev_need(enc->vals, &B->vals, W * 64 * (size_t)G.value_bytes, kPqJob, "compacted values"));
  JOB_TRY(dev_need(enc->isz, &B->isz, I, kPqJob, "item sizes"));
  JOB_TRY(dev_need(enc->ioff, &B->ioff, I + 1, kPqJob, "item offsets"));
  JOB_TRY(dev_need(enc->part, &B->part, std::max(W, I) / samk::kScanChunk + 3, kPqJob, "scan partials"));
  HIP_TRY(enc->clock.mark(PQ_SIZE_0, s));
  *live = true;
  return BQSR_OK;
}
bqsr_status pq_finish(bqsr_parquet_pages* enc, const PqScratch& B, hipStream_t s, bqsr_parquet_pages_sizes* out) {
  const pqk::Geo& G = enc->G;
  JOB_TRY(sam_scan(B.isz, G.n_items, B.ioff, B.part, s));
  HIP_TRY(enc->clock.mark(PQ_SIZE_1, s));
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, B.ioff + G.n_items, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  enc->clock.add(g_pq_ms[PQ_SIZE], PQ_SIZE_0, PQ_SIZE_1);
  enc->body_bytes = (int64_t)total;
  out->body_bytes = enc->body_bytes;
  enc->sized = true;
  return BQSR_OK;
}
// the passes of a string or boolean column between pq_begin and pq_finish
bqsr_status pq_size_bytes(bqsr_parquet_pages* enc, const PqScratch& B, const uint64_t* validity, const uint64_t* bits,
                          const int32_t* offsets, hipStream_t s) {
  const pqk::Geo& G = enc->G;
  const int cap = enc->ctx->tune_pileup_grid > 0 ? enc->ctx->tune_pileup_grid : enc->ctx->n_cu * 8;
  JOB_TRY(launch(pqk::pq_bitmap_levels, sam_grid(G.n_words, pqk::kThreads, cap), pqk::kThreads, s, validity, G, B.vword,
                 B.cnt));
  JOB_TRY(sam_scan(B.cnt, G.n_words, B.voff, B.part, s));
  JOB_TRY(launch(pqk::pq_compact_bytes, pq_grid(enc->ctx, G.n_words), pqk::kThreads, s, G, (const uint64_t*)B.vword,
                 (const uint64_t*)B.voff, bits, (void*)B.vals));
  JOB_TRY(launch(pqk::pq_items_bytes, pq_grid(enc->ctx, G.n_items), pqk::kThreads, s, G, (const uint64_t*)B.voff,
                 (const void*)B.vals, offsets, B.isz));
  return BQSR_OK;
}
// the launch half of an emit (rows at all): the write pass into the handle's device buffers, between the emit
// stage's marks.  The bodies are readable to their end rounded up to 4 (the codec reads aligned words).
bqsr_status pq_emit_launch(bqsr_parquet_pages* enc, hipStream_t s, uint8_t** out_p, bqsr_parquet_page** ptab_p) {
  const pqk::Geo& G = enc->G;
  uint8_t* out;
  bqsr_parquet_page* ptab;
  JOB_TRY(dev_need(enc->out, &out, (size_t)enc->body_bytes + 64, kPqJob, "page bodies"));
  JOB_TRY(dev_need(enc->ptab, &ptab, (size_t)G.n_pages, kPqJob, "page table"));
  HIP_TRY(enc->clock.mark(PQ_EMIT_0, s));
  if (G.kind == BQSR_PARQUET_PLAIN_BYTE_ARRAY || G.kind == BQSR_PARQUET_PLAIN_BOOLEAN) {
    JOB_TRY(launch(pqk::pq_emit_bytes, pq_grid(enc->ctx, G.n_items), pqk::kThreads, s, G,
                   (const uint64_t*)enc->vword.p, (const uint64_t*)enc->voff.p, (const void*)enc->vals.p, enc->s_off,
                   enc->s_bytes, (const uint64_t*)enc->ioff.p, out, ptab));
  } else {
    JOB_TRY(launch(pqk::pq_emit, pq_grid(enc->ctx, G.n_items), pqk::kThreads, s, G, (const uint64_t*)enc->vword.p,
                   (const uint64_t*)enc->voff.p, (const void*)enc->vals.p, (const uint64_t*)enc->ioff.p, out, ptab));
  }
  HIP_TRY(enc->clock.mark(PQ_EMIT_1, s));
  *out_p = out;
  *ptab_p = ptab;
  return BQSR_OK;
}

}  // namespace

extern "C" {

bqsr_status bqsr_parquet_pages_create(bqsr_context* ctx, bqsr_parquet_pages** out) {
  if (!ctx || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_parquet_pages_create: bad arguments");
  bqsr_parquet_pages* e = new (std::nothrow) bqsr_parquet_pages;
  if (!e) return fail(BQSR_ERR_DEVICE, "bqsr_parquet_pages_create: out of memory");
  e->ctx = ctx;
  *out = e;
  return ok();
}

void bqsr_parquet_pages_destroy(bqsr_parquet_pages* enc) { delete enc; }

bqsr_status bqsr_parquet_pages_size(bqsr_parquet_pages* enc, const bqsr_parquet_column* col, int64_t n_rows,
                                    int64_t page_rows, void* stream, bqsr_parquet_pages_sizes* out) {
  if (!enc || !out || page_rows <= 0 || page_rows % 64 || page_rows > (1 << 24))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_parquet_pages_size: bad arguments (page_rows is a multiple of 64)");
  JOB_TRY(pq_check(col, n_rows, "bqsr_parquet_pages_size"));
  hipStream_t s = S(stream);
  PqScratch B;
  bool live;
  JOB_TRY(pq_begin(enc, n_rows, page_rows, col->kind, col->kind == BQSR_PARQUET_PLAIN_INT64 ? 8 : 4,
                   col->kind == BQSR_PARQUET_DICT_INDEX ? col->bit_width : 32, s, out, "bqsr_parquet_pages_size", &B,
                   &live));
  if (!live) return ok();
  const pqk::Geo& G = enc->G;
  JOB_TRY(launch(pqk::pq_levels, pq_grid(enc->ctx, G.n_words), pqk::kThreads, s, *col, G, B.vword, B.cnt));
  JOB_TRY(sam_scan(B.cnt, G.n_words, B.voff, B.part, s));
  JOB_TRY(launch(pqk::pq_compact, pq_grid(enc->ctx, G.n_words), pqk::kThreads, s, *col, G, (const uint64_t*)B.vword,
                 (const uint64_t*)B.voff, (void*)B.vals));
  JOB_TRY(launch(pqk::pq_items, pq_grid(enc->ctx, G.n_items), pqk::kThreads, s, G, (const uint64_t*)B.voff,
                 (const void*)B.vals, B.isz));
  JOB_TRY(pq_finish(enc, B, s, out));
  return ok();
}

bqsr_status bqsr_parquet_pages_size_strings(bqsr_parquet_pages* enc, const int32_t* offsets, const uint8_t* bytes,
                                            const uint64_t* validity, int64_t n_rows, int64_t page_rows, void* stream,
                                            bqsr_parquet_pages_sizes* sizes) {
  const char* who = "bqsr_parquet_pages_size_strings";
  hipStream_t s = S(stream);
  PqScratch B;
  bool live;
  if (n_rows > 0 && (!offsets || !bytes))
    return fail(BQSR_ERR_INVALID_ARG, std::string(who) + ": the source does not cover the rows");
  JOB_TRY(pq_begin(enc, n_rows, page_rows, BQSR_PARQUET_PLAIN_BYTE_ARRAY, 4, 32, s, sizes, who, &B, &live));
  enc->s_off = offsets;
  enc->s_bytes = bytes;
  if (!live) return ok();
  JOB_TRY(pq_size_bytes(enc, B, validity, nullptr, offsets, s));
  JOB_TRY(pq_finish(enc, B, s, sizes));
  return ok();
}

bqsr_status bqsr_parquet_pages_size_bools(bqsr_parquet_pages* enc, const uint64_t* bits, const uint64_t* validity,
                                          int64_t n_rows, int64_t page_rows, void* stream,
                                          bqsr_parquet_pages_sizes* sizes) {
  const char* who = "bqsr_parquet_pages_size_bools";
  hipStream_t s = S(stream);
  PqScratch B;
  bool live;
  if (n_rows > 0 && !bits) return fail(BQSR_ERR_INVALID_ARG, std::string(who) + ": the source does not cover the rows");
  JOB_TRY(pq_begin(enc, n_rows, page_rows, BQSR_PARQUET_PLAIN_BOOLEAN, 1, 32, s, sizes, who, &B, &live));
  if (!live) return ok();
  JOB_TRY(pq_size_bytes(enc, B, validity, bits, nullptr, s));
  JOB_TRY(pq_finish(enc, B, s, sizes));
  return ok();
}

bqsr_status bqsr_parquet_pages_emit(bqsr_parquet_pages* enc, uint8_t* bodies, bqsr_parquet_page* pages, void* stream) {
  if (!enc) return fail(BQSR_ERR_INVALID_ARG, "bqsr_parquet_pages_emit: bad arguments");
  if (!enc->sized) return fail(BQSR_ERR_INVALID_ARG, "bqsr_parquet_pages_emit before bqsr_parquet_pages_size");
  enc->sized = false;  // (one emit per size call: the scratch is the next column's)
  g_pq_ms[PQ_EMIT] = 0.0;
  const pqk::Geo& G = enc->G;
  if (G.n_rows == 0) return ok();
  if (!bodies || !pages) return fail(BQSR_ERR_INVALID_ARG, "bqsr_parquet_pages_emit: bad arguments");
  HIP_TRY(hipSetDevice(enc->ctx->device));
  hipStream_t s = S(stream);
  uint8_t* out;
  bqsr_parquet_page* ptab;
  JOB_TRY(pq_emit_launch(enc, s, &out, &ptab));
  HIP_TRY(hipMemcpyAsync(bodies, out, (size_t)enc->body_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(pages, ptab, (size_t)G.n_pages * sizeof(bqsr_parquet_page), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  enc->clock.add(g_pq_ms[PQ_EMIT], PQ_EMIT_0, PQ_EMIT_1);
  return ok();
}

bqsr_status bqsr_parquet_pages_minmax(bqsr_parquet_pages* enc, const bqsr_parquet_column* col, int64_t n_rows,
                                      void* stream, int64_t* min_out, int64_t* max_out, int64_t* non_nulls) {
  if (!enc || !min_out || !max_out || !non_nulls)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_parquet_pages_minmax: bad arguments");
  JOB_TRY(pq_check(col, n_rows, "bqsr_parquet_pages_minmax"));
  long long h[3] = {INT64_MAX, INT64_MIN, 0};
  if (n_rows) {
    HIP_TRY(hipSetDevice(enc->ctx->device));
    hipStream_t s = S(stream);
    long long* mm;
    JOB_TRY(dev_need(enc->mm, &mm, 3, kPqJob, "min / max"));
    HIP_TRY(hipMemcpyAsync(mm, h, sizeof h, hipMemcpyHostToDevice, s));
    JOB_TRY(launch(pqk::pq_minmax, sam_grid(n_rows, pqk::kThreads, enc->ctx->n_cu * 8), pqk::kThreads, s, *col, n_rows,
                   mm));
    HIP_TRY(hipMemcpyAsync(h, mm, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  *min_out = h[0];
  *max_out = h[1];
  *non_nulls = h[2];
  return ok();
}

bqsr_status bqsr_parquet_pages_kernel_times(double* size_ms, double* emit_ms) {
  if (size_ms) *size_ms = g_pq_ms[PQ_SIZE];
  if (emit_ms) *emit_ms = g_pq_ms[PQ_EMIT];
  return BQSR_OK;
}

}  // extern "C"
