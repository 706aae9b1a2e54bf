// snappy_pages.hip -- Parquet page bodies compressed with snappy on the
// device: what parquet_pages.py's writer threads do with pyarrow.compress.
//
// The format is declared in include/adam_sam.h (bqsr_snappy_pages): a page of
// n bytes is varint(n) and then the elements of its ceil(n / 65536) blocks,
// every block compressed on its own, so a page of any size is a set of
// independent workgroup-sized jobs.  A persistent grid takes one (page, block)
// job at a time, as bgzf_deflate_kernel takes members (one workgroup a CU: see
// the LDS below), and
//   1. stages the block's bytes in LDS (the source is at any byte offset:
//      aligned words are read and funnel-shifted);
//   2. goes through it in chunks of kChunk positions with bgzf_deflate.hip's
//      scheme -- three candidates per position (distance 1, the bucket's first
//      position of this chunk, the bucket's highest position of the earlier
//      chunks), winners by position, never by timing; the greedy path marked
//      by pointer doubling -- with two changes: a match is at least 4 and at
//      most 64 bytes, so it is exactly one copy element.  The path's
//      positions are compacted into 32-bit tokens in global memory (the whole
//      block's: a literal run may span chunks), a literal with the number of
//      copies before it, and every copy's token index into a table beside them;
//   3. emits: a literal token whose predecessor is a copy (or none) heads a
//      run, and the run ends at the next copy's token index (the segmented scan
//      of the run lengths, read from the copies' table); every token's element
//      bytes (a head's with its run's tag and length bytes), a workgroup scan,
//      and every lane writes its tokens' bytes into the block's slot: a byte of
//      the output belongs to one lane.
// The blocks' sizes and each page's varint are scanned and snappy_pack_kernel
// writes the varints and moves the slots to their final offsets: only the
// packed buffer and the (offset, bytes) table are downloaded.
//
// A slot holds every parse under the rules: a copy emits at most 3 bytes for at
// least 4 bytes of input, and a literal run of L bytes emits L + 1 bytes up to
// 60, L + 2 up to 256 and L + 3 beyond.  Two runs are separated by a copy, so
// charge each run's tag bytes beyond the first to the pair (run, copy after
// it): the pair emits at most L + 3 + 3 bytes for L + 4 of input when L > 256
// (2 more, once per 261 bytes at most), L + 2 + 3 for L + 4 when L > 60 (1
// more, once per 65 bytes at most), and no more than its input otherwise.  A
// block of n bytes therefore emits at most n + n / 65 + 3 bytes (the last run
// has no copy behind it), below kSlot = 32 + 65536 + 65536 / 6 rounded up.
//
// LDS: 65632 bytes of input, 2 * 32768 of hash tables (13 bits: a bucket keeps
// one position per table, and with deflate's 12 bits a repeat at a distance of
// a few thousand bytes was shadowed by a colliding position about every other
// time), 8192 + 8200 + 2056 of the chunk's matches, jumps and marks, 2088 of
// scan: 148 KB of the CU's 160, one workgroup a CU, as for deflate.
//
// The block routine is phases between barriers (bgzf_deflate.hip's DFL_FOR_T ..
// DFL_SYNC) with order-independent cross-lane updates, so the same source
// compiles for the host: bqsr_snappy_pages_host gives the device's bytes.
// Shared with bgzf_deflate.hip: the phase macros, the min / max updates, the
// workgroup scan, ld4 / extend.  The match and path phases themselves
// are a specialised copy (minimum 4 for the run candidate too, the cap of 64,
// no histograms, another token format).
//
// Included by bqsr_capi.cpp after parquet_pages.hip.

namespace snpk {

using dflk::kThreads;
constexpr int kBlock = 65536;                      // bytes of a page per block
constexpr int kSlot = 76544;                       // 32 + 65536 + 65536 / 6 = 76490, rounded up to 256
constexpr int kChunk = 2048;                       // positions per matching / parsing round
constexpr int kPer = kChunk / kThreads;
constexpr int kHashBits = 13;
constexpr int kInWords = kBlock / 4 + 24;          // (a match is compared up to 64 bytes past the block's end)
constexpr int kMinMatch = 4, kMaxMatch = 64;
constexpr int kMaxCopies = kBlock / kMinMatch;
constexpr int kTokWords = kBlock + kMaxCopies + 8;  // a workgroup's scratch: the tokens, then the copies' token indices
static_assert(kChunk % kThreads == 0 && kChunk > kMaxMatch, "a match never jumps over a whole chunk");
static_assert(kBlock / kChunk <= 32, "the chunk tag of `first`");
static_assert(kSlot >= 32 + kBlock + kBlock / 6 && kSlot % 4 == 0, "the slot");

struct Lds {
  uint32_t in32[kInWords];          // the block's bytes (zeros behind them)
  uint32_t head[1 << kHashBits];    // per bucket: the highest inserted position + 1, 0 none
  uint32_t first[1 << kHashBits];   // per bucket: (31 - chunk) << 16 | the chunk's lowest position
  uint32_t m[kChunk];               // per position of the chunk: len << 16 | distance - 1
  uint16_t jmp[2][kChunk + 2];      // pointer doubling; [cl] is the chunk's exit
  uint8_t mark[kChunk + 8];
  uint32_t scan[kThreads];
  uint32_t wsum[kThreads / 64];
  uint32_t scan_total;
  uint32_t e_next;
};

// a (page, block) job: the block's bytes in the input, and the item of the size table it answers to
struct Job {
  uint64_t src;
  uint32_t n;
  uint32_t item;
};
// a page: its size (the varint) and its first item
struct Page {
  uint64_t n;
  uint64_t item;
};

__host__ __device__ __forceinline__ uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }
__host__ __device__ __forceinline__ int varint_len(uint64_t v) {
  int k = 1;
  while (v >= 128 && k < 10) v >>= 7, ++k;
  return k;
}
__host__ __device__ __forceinline__ uint32_t lit_tag_bytes(uint32_t L) { return L <= 60 ? 1u : L <= 256 ? 2u : 3u; }

// tokens: a copy is 1 << 31 | offset << 8 | length; a literal its byte | copies before it << 8
__host__ __device__ __forceinline__ bool tok_copy(uint32_t tok) { return (tok >> 31) != 0; }
// the element bytes token j adds: a copy's 2 or 3; a literal's 1, and for the head of a run the run's tag and
// length bytes too (*run: the run's length for a head, else 0)
__host__ __device__ __forceinline__ uint32_t tok_bytes(const uint32_t* gtok, const uint32_t* cpos, uint32_t j,
                                                       uint32_t ntok, uint32_t ncopy, uint32_t tok, uint32_t* run) {
  *run = 0;
  if (tok_copy(tok)) return (tok & 127u) <= 11u && ((tok >> 8) & 0xFFFFu) < 2048u ? 2u : 3u;
  if (j != 0 && !tok_copy(gtok[j - 1])) return 1u;
  const uint32_t c = (tok >> 8) & 0x7FFFu;  // the run ends at the next copy's token
  const uint32_t end = c < ncopy ? cpos[c] : ntok;
  *run = end - j;
  return 1u + lit_tag_bytes(*run);
}

// One block: gin[0, n) (1 <= n <= kBlock, any byte offset; on the device the
// aligned words that hold it are read) into slot (kSlot bytes), its size into
// *size.  gtok: kTokWords words of scratch.
__host__ __device__ inline void snappy_block(Lds& S, const uint8_t* gin, int n, uint32_t* gtok, uint8_t* slot,
                                             uint64_t* size) {
  const uint8_t* in8 = (const uint8_t*)S.in32;
  uint32_t* cpos = gtok + kBlock;
  // ---- 1. the bytes into LDS, the tables cleared ----
  DFL_FOR_T {
#if defined(__HIP_DEVICE_COMPILE__)
    const int a = (int)((uintptr_t)gin & 3u), sh = a * 8;
    const uint32_t* w = (const uint32_t*)(gin - a);
    const int nw = (a + n + 3) >> 2;  // the aligned words that hold a byte of the block
#endif
    for (int i = t; i < kInWords; i += kThreads) {
      uint32_t v = 0;
      const int rem = n - 4 * i;
      if (rem > 0) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t lo = w[i], hi = a && i + 1 < nw ? w[i + 1] : 0u;
        v = a ? (lo >> sh) | (hi << (32 - sh)) : lo;
        if (rem < 4) v &= (1u << (8 * rem)) - 1u;
#else
        for (int k = 0; k < 4 && k < rem; ++k) v |= (uint32_t)gin[4 * (size_t)i + k] << (8 * k);
#endif
      }
      S.in32[i] = v;
    }
    for (int i = t; i < (1 << kHashBits); i += kThreads) S.head[i] = 0, S.first[i] = 0xFFFFFFFFu;
  }
  DFL_SYNC();
  // ---- 2. matches and the greedy parse, a chunk at a time ----
  int e = 0;  // the parse's next position
  uint32_t ntok = 0, ncopy = 0;
  for (int c0 = 0; c0 < n; c0 += kChunk) {
    const int cl = n - c0 < kChunk ? n - c0 : kChunk;
    const uint32_t ctag = (uint32_t)(31 - c0 / kChunk) << 16;
    DFL_FOR_T {
      for (int i = t; i < cl; i += kThreads)
        if (n - (c0 + i) >= 4) dflk::dfl_min(&S.first[hash4(dflk::ld4(S, c0 + i))], ctag | (uint32_t)i);
    }
    DFL_SYNC();
    DFL_FOR_T {
      for (int i = t; i < cl; i += kThreads) {
        const int p = c0 + i;
        const int maxlen = n - p < kMaxMatch ? n - p : kMaxMatch;
        int best = 0, bd = 0;
        if (maxlen >= kMinMatch) {
          if (p >= 1) {  // a run
            const int l = dflk::extend(S, p, p - 1, maxlen);
            if (l >= kMinMatch) best = l, bd = 1;
          }
          const uint32_t h = hash4(dflk::ld4(S, p));
          const uint32_t f = S.first[h];  // the bucket's first position of this chunk, when it is before p
          if ((f & 0xFFFF0000u) == ctag && (int)(f & 0xFFFFu) < i && i - (int)(f & 0xFFFFu) > 1) {
            const int l = dflk::extend(S, p, c0 + (int)(f & 0xFFFFu), maxlen);
            if (l >= kMinMatch && l > best) best = l, bd = i - (int)(f & 0xFFFFu);
          }
          const uint32_t q1 = S.head[h];
          const int d = p - (int)q1 + 1;
          if (q1 != 0 && d > 1 && d <= 65535) {
            const int l = dflk::extend(S, p, p - d, maxlen);
            if (l >= kMinMatch && l > best) best = l, bd = d;
          }
        }
        S.m[i] = ((uint32_t)best << 16) | (uint32_t)(bd ? bd - 1 : 0);
        const int nx = i + (best ? best : 1);
        S.jmp[0][i] = (uint16_t)(nx < cl ? nx : cl);
      }
      if (t == 0) S.jmp[0][cl] = S.jmp[1][cl] = (uint16_t)cl;
    }
    DFL_SYNC();
    DFL_FOR_T {
      for (int i = t; i < cl; i += kThreads) {
        const int p = c0 + i;
        if (n - p >= 4) dflk::dfl_max(&S.head[hash4(dflk::ld4(S, p))], (uint32_t)p + 1u);
        S.mark[i] = p == e;
      }
    }
    DFL_SYNC();
    // the positions on the path from e: after round r every one within 2^(r+1) steps is marked
    int cur = 0;
    for (int r = 0; r < 12 && (1 << r) < cl; ++r, cur ^= 1) {
      DFL_FOR_T {
        for (int i = t; i < cl; i += kThreads) {
          const int j = S.jmp[cur][i];  // <= cl
          if (S.mark[i] && j < cl) S.mark[j] = 1;
          S.jmp[cur ^ 1][i] = S.jmp[cur][j];
        }
      }
      DFL_SYNC();
    }
    DFL_FOR_T {  // the path's positions, and its copies in the high half
      uint32_t c = 0;
      for (int k = 0; k < kPer; ++k) {
        const int i = t * kPer + k;
        if (i < cl && S.mark[i]) c += 1u + ((S.m[i] >> 16) ? 0x10000u : 0u);
      }
      S.scan[t] = c;
    }
    DFL_SYNC();
    dflk::dfl_scan(S);
    DFL_FOR_T {
      uint32_t at = ntok + (S.scan[t] & 0xFFFFu), cc = ncopy + (S.scan[t] >> 16);
      for (int k = 0; k < kPer; ++k) {
        const int i = t * kPer + k;
        if (i >= cl || !S.mark[i]) continue;
        const uint32_t mm = S.m[i];
        const int len = (int)(mm >> 16);
        uint32_t tok;
        if (len) {
          tok = 0x80000000u | (((mm & 0xFFFFu) + 1u) << 8) | (uint32_t)len;
          if (cc < (uint32_t)kMaxCopies) cpos[cc] = at;
          ++cc;
        } else {
          tok = (uint32_t)in8[c0 + i] | (cc << 8);
        }
        if (at < (uint32_t)kBlock) gtok[at] = tok;
        ++at;
        const int nx = i + (len ? len : 1);
        if (nx >= cl) S.e_next = (uint32_t)(c0 + nx);  // (one position of a path leaves the chunk)
      }
    }
    DFL_SYNC();
    if (S.scan_total) {
      e = (int)S.e_next;
      ntok += S.scan_total & 0xFFFFu;
      ncopy += S.scan_total >> 16;
    }
  }
  if (ntok > (uint32_t)kBlock) ntok = kBlock;
  if (ncopy > (uint32_t)kMaxCopies) ncopy = kMaxCopies;
  // ---- 3. the elements ----
  uint32_t base = 0;
  for (uint32_t g0 = 0; g0 < ntok; g0 += kChunk) {
    DFL_FOR_T {
      uint32_t c = 0, run;
      for (int k = 0; k < kPer; ++k) {
        const uint32_t j = g0 + (uint32_t)(t * kPer + k);
        if (j < ntok) c += tok_bytes(gtok, cpos, j, ntok, ncopy, gtok[j], &run);
      }
      S.scan[t] = c;
    }
    DFL_SYNC();
    dflk::dfl_scan(S);
    DFL_FOR_T {
      uint32_t o = base + S.scan[t];
      auto put = [&](uint32_t b) {
        if (o < (uint32_t)kSlot) slot[o] = (uint8_t)b;
        ++o;
      };
      for (int k = 0; k < kPer; ++k) {
        const uint32_t j = g0 + (uint32_t)(t * kPer + k);
        if (j >= ntok) break;
        const uint32_t tok = gtok[j];
        uint32_t run;
        const uint32_t nb = tok_bytes(gtok, cpos, j, ntok, ncopy, tok, &run);
        if (tok_copy(tok)) {
          const uint32_t len = tok & 127u, off = (tok >> 8) & 0xFFFFu;
          if (nb == 2) {
            put(1u | ((len - 4u) << 2) | ((off >> 8) << 5));
            put(off & 0xFFu);
          } else {
            put(2u | ((len - 1u) << 2));
            put(off & 0xFFu);
            put(off >> 8);
          }
          continue;
        }
        if (run) {
          if (run <= 60) {
            put((run - 1u) << 2);
          } else if (run <= 256) {
            put(60u << 2);
            put(run - 1u);
          } else {
            put(61u << 2);
            put((run - 1u) & 0xFFu);
            put((run - 1u) >> 8);
          }
        }
        put(tok & 0xFFu);
      }
    }
    DFL_SYNC();
    base += S.scan_total;
  }
  DFL_FOR_T {
    if (t == 0) *size = base < (uint32_t)kSlot ? base : (uint32_t)kSlot;
  }
  DFL_SYNC();
}

extern "C" __global__ void __launch_bounds__(kThreads) snappy_blocks_kernel(const uint8_t* in, const Job* jobs,
                                                                           int64_t njobs, uint32_t* tok,
                                                                           uint8_t* slots, uint64_t* sizes) {
  __shared__ Lds S;
  for (int64_t j = blockIdx.x; j < njobs; j += gridDim.x) {  // (uniform over the workgroup)
    const Job jb = jobs[j];
    const int n = (int)(jb.n < (uint32_t)kBlock ? jb.n : (uint32_t)kBlock);
    if (n <= 0) continue;
    snappy_block(S, in + jb.src, n, tok + (int64_t)blockIdx.x * kTokWords, slots + j * kSlot, sizes + jb.item);
  }
}

// a page's varint at out + off[its first item] (a lane a page), and the slots' blocks one after another behind it:
// out + off[the job's item], dwords once the destination is aligned
extern "C" __global__ void __launch_bounds__(256) snappy_pack_kernel(const uint8_t* slots, const Job* jobs, int64_t njobs,
                                                                     const Page* pages, int64_t n_pages,
                                                                     const uint64_t* sizes, const uint64_t* off,
                                                                     uint8_t* out) {
  for (int64_t p = blockIdx.x * (int64_t)256 + threadIdx.x; p < n_pages; p += (int64_t)gridDim.x * 256) {
    uint64_t v = pages[p].n;
    uint8_t* o = out + off[pages[p].item];
    const int nb = varint_len(v);
    for (int k = 0; k < nb; ++k, v >>= 7) o[k] = (uint8_t)((v & 127u) | (k + 1 < nb ? 128u : 0u));
  }
  for (int64_t m = blockIdx.x; m < njobs; m += gridDim.x) {
    const uint32_t item = jobs[m].item;
    const uint8_t* src = slots + m * kSlot;
    const uint32_t* s32 = (const uint32_t*)src;  // (kSlot % 4 == 0)
    const int sz = (int)(sizes[item] < (uint64_t)kSlot ? sizes[item] : (uint64_t)kSlot);
    uint8_t* o = out + off[item];
    const int t = threadIdx.x;
    const int a = (int)((4u - ((uintptr_t)o & 3u)) & 3u), head = a < sz ? a : sz;
    if (t < head) o[t] = src[t];
    const int nw = (sz - head) >> 2;
    uint32_t* o32 = (uint32_t*)(o + head);
    for (int i = t; i < nw; i += 256) {
      const int q = head + 4 * i, s = (q & 3) * 8;
      o32[i] = s ? (s32[q >> 2] >> s) | (s32[(q >> 2) + 1] << (32 - s)) : s32[q >> 2];
    }
    for (int i = head + 4 * nw + t; i < sz; i += 256) o[i] = src[i];
  }
}

}  // namespace snpk

namespace {

enum { SNAPPY_BLOCKS, SNAPPY_PACK, SNAPPY_STAGES };
enum { SNAPPY_BLOCKS_0, SNAPPY_BLOCKS_1, SNAPPY_PACK_0, SNAPPY_PACK_1 };
thread_local double g_snappy_ms[SNAPPY_STAGES] = {0.0, 0.0};
const char* kSnappyJob = "snappy pages";

// the pages of one call cut into jobs, and the size table's first state: a page's varint length at its first item,
// its blocks' items behind it
struct SnappyPlan {
  std::vector<snpk::Job> jobs;
  std::vector<snpk::Page> pages;
  std::vector<uint64_t> sizes;
  void add_page(uint64_t src, uint64_t n) {
    pages.push_back(snpk::Page{n, (uint64_t)sizes.size()});
    sizes.push_back((uint64_t)snpk::varint_len(n));
    for (uint64_t a = 0; a < n; a += snpk::kBlock) {
      jobs.push_back(snpk::Job{src + a, (uint32_t)std::min<uint64_t>(snpk::kBlock, n - a), (uint32_t)sizes.size()});
      sizes.push_back(0);
    }
  }
};

// the device scratch of the compressor (an encoder handle keeps one across calls) and its clock
struct SnappyBufs {
  DevBuf jobs, pages, sizes, off, part, tok, slots, packed;
  StageClock<4> clock;
};

// d_in (device memory; readable from its 4-byte aligned start to its end rounded up to 4) holds the plan's pages:
// compressed, packed into B.packed, the items' offsets into `off` (the plan's items + 1: the last is the total)
bqsr_status snappy_device(bqsr_context* ctx, const uint8_t* d_in, const SnappyPlan& P, hipStream_t s, SnappyBufs& B,
                          std::vector<uint64_t>& off) {
  g_snappy_ms[SNAPPY_BLOCKS] = g_snappy_ms[SNAPPY_PACK] = 0.0;
  const int64_t njobs = (int64_t)P.jobs.size(), n_pages = (int64_t)P.pages.size(), n_items = (int64_t)P.sizes.size();
  off.assign((size_t)n_items + 1, 0);
  if (n_pages == 0) return BQSR_OK;
  if (n_items >= (int64_t)UINT32_MAX) return fail(BQSR_ERR_INVALID_ARG, "snappy pages: too many blocks in one call");
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(njobs, (int64_t)ctx->n_cu));
  snpk::Job* d_jobs;
  snpk::Page* d_pages;
  uint64_t *d_sizes, *d_off, *d_part;
  uint32_t* d_tok;
  uint8_t *d_slots, *d_packed;
  JOB_TRY(dev_need(B.jobs, &d_jobs, (size_t)njobs, kSnappyJob, "jobs"));
  JOB_TRY(dev_need(B.pages, &d_pages, (size_t)n_pages, kSnappyJob, "pages"));
  JOB_TRY(dev_need(B.sizes, &d_sizes, (size_t)n_items, kSnappyJob, "item sizes"));
  JOB_TRY(dev_need(B.off, &d_off, (size_t)n_items + 1, kSnappyJob, "item offsets"));
  JOB_TRY(dev_need(B.part, &d_part, (size_t)(n_items / samk::kScanChunk + 3), kSnappyJob, "scan partials"));
  JOB_TRY(dev_need(B.tok, &d_tok, (size_t)grid * snpk::kTokWords, kSnappyJob, "tokens"));
  JOB_TRY(dev_need(B.slots, &d_slots, (size_t)njobs * snpk::kSlot + 64, kSnappyJob, "block slots"));
  if (njobs) HIP_TRY(hipMemcpyAsync(d_jobs, P.jobs.data(), (size_t)njobs * sizeof(snpk::Job), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_pages, P.pages.data(), (size_t)n_pages * sizeof(snpk::Page), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_sizes, P.sizes.data(), (size_t)n_items * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(B.clock.mark(SNAPPY_BLOCKS_0, s));
  if (njobs)
    JOB_TRY(launch(snpk::snappy_blocks_kernel, grid, snpk::kThreads, s, d_in, (const snpk::Job*)d_jobs, njobs, d_tok,
                   d_slots, d_sizes));
  HIP_TRY(B.clock.mark(SNAPPY_BLOCKS_1, s));
  JOB_TRY(sam_scan(d_sizes, n_items, d_off, d_part, s));
  HIP_TRY(hipMemcpyAsync(off.data(), d_off, off.size() * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // (the plan's vectors were read by the copies)
  const uint64_t total = off[(size_t)n_items];
  if (total > (uint64_t)njobs * snpk::kSlot + (uint64_t)n_pages * 10)
    return fail(BQSR_ERR_DEVICE, "snappy pages: block sizes out of range");
  JOB_TRY(dev_need(B.packed, &d_packed, (size_t)total + 64, kSnappyJob, "packed pages"));
  HIP_TRY(B.clock.mark(SNAPPY_PACK_0, s));
  JOB_TRY(launch(snpk::snappy_pack_kernel,
                 (unsigned)std::max<int64_t>(1, std::min<int64_t>(std::max(njobs, (n_pages + 255) / 256),
                                                                  (int64_t)ctx->n_cu * 8)),
                 256, s, (const uint8_t*)d_slots, (const snpk::Job*)d_jobs, njobs, (const snpk::Page*)d_pages, n_pages,
                 (const uint64_t*)d_sizes, (const uint64_t*)d_off, d_packed));
  HIP_TRY(B.clock.mark(SNAPPY_PACK_1, s));
  HIP_TRY(hipStreamSynchronize(s));
  B.clock.add(g_snappy_ms[SNAPPY_BLOCKS], SNAPPY_BLOCKS_0, SNAPPY_BLOCKS_1);
  B.clock.add(g_snappy_ms[SNAPPY_PACK], SNAPPY_PACK_0, SNAPPY_PACK_1);
  return BQSR_OK;
}

// the pages' offsets in the packed output from the items' (out_off: the plan's pages + 1)
void snappy_page_offsets(const SnappyPlan& P, const std::vector<uint64_t>& off, int64_t* out_off) {
  for (size_t p = 0; p < P.pages.size(); ++p) out_off[p] = (int64_t)off[(size_t)P.pages[p].item];
  out_off[P.pages.size()] = (int64_t)off[P.sizes.size()];
}

bqsr_status snappy_check(const uint8_t* in, const int64_t* page_off, int64_t n_pages, const uint8_t* out, int64_t cap,
                         const int64_t* out_off, const char* who) {
  const std::string w(who);
  if (n_pages < 0 || !page_off || !out_off || cap < 0 || (cap > 0 && !out))
    return fail(BQSR_ERR_INVALID_ARG, w + ": bad arguments");
  if (page_off[0] < 0) return fail(BQSR_ERR_INVALID_ARG, w + ": page offsets must not be negative");
  for (int64_t p = 0; p < n_pages; ++p)
    if (page_off[p + 1] < page_off[p] || page_off[p + 1] - page_off[p] > (int64_t)INT32_MAX)
      return fail(BQSR_ERR_INVALID_ARG, w + ": page offsets must not decrease, and a page is below 2^31 bytes");
  if (page_off[n_pages] > page_off[0] && !in) return fail(BQSR_ERR_INVALID_ARG, w + ": bad arguments");
  return BQSR_OK;
}

}  // namespace

extern "C" {

bqsr_status bqsr_snappy_pages(bqsr_context* ctx, const uint8_t* in, const int64_t* page_off, int64_t n_pages,
                              void* stream, uint8_t* out, int64_t cap, int64_t* out_off) {
  if (!ctx) return fail(BQSR_ERR_INVALID_ARG, "bqsr_snappy_pages: bad arguments");
  JOB_TRY(snappy_check(in, page_off, n_pages, out, cap, out_off, "bqsr_snappy_pages"));
  out_off[0] = 0;
  if (n_pages == 0) return ok();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  // the bytes from the first page's start to the last page's end, at their offset modulo 4
  const int64_t lo = page_off[0], n = page_off[n_pages] - lo, pad = lo & 3;
  SnappyPlan P;
  for (int64_t p = 0; p < n_pages; ++p)
    P.add_page((uint64_t)(page_off[p] - lo + pad), (uint64_t)(page_off[p + 1] - page_off[p]));
  SnappyBufs B;
  DevBuf din;
  uint8_t* d_in;
  JOB_TRY(dev_need(din, &d_in, (size_t)(n + pad) + 64, kSnappyJob, "input"));
  if (n > 0) JOB_TRY(upload_staged(ctx, d_in + pad, in + lo, (size_t)n, s));
  std::vector<uint64_t> off;
  JOB_TRY(snappy_device(ctx, d_in, P, s, B, off));
  snappy_page_offsets(P, off, out_off);
  const int64_t total = out_off[n_pages];
  if (total > cap) return fail(BQSR_ERR_INVALID_ARG, "bqsr_snappy_pages: the output does not fit (see out_off[n_pages])");
  if (total > 0) HIP_TRY(hipMemcpy(out, B.packed.p, (size_t)total, hipMemcpyDeviceToHost));
  return ok();
}

bqsr_status bqsr_snappy_pages_host(const uint8_t* in, const int64_t* page_off, int64_t n_pages, uint8_t* out,
                                   int64_t cap, int64_t* out_off) {
  JOB_TRY(snappy_check(in, page_off, n_pages, out, cap, out_off, "bqsr_snappy_pages_host"));
  out_off[0] = 0;
  if (n_pages == 0) return ok();
  std::unique_ptr<snpk::Lds> S(new (std::nothrow) snpk::Lds);
  if (!S) return fail(BQSR_ERR_DEVICE, "bqsr_snappy_pages_host: out of host memory");
  std::vector<uint32_t> tok((size_t)snpk::kTokWords);
  std::vector<uint8_t> slot((size_t)snpk::kSlot);
  int64_t at = 0;
  bool fits = true;
  auto put = [&](const uint8_t* p, int64_t k) {
    if (fits && at + k <= cap) memcpy(out + at, p, (size_t)k);
    else fits = false;
    at += k;
  };
  for (int64_t p = 0; p < n_pages; ++p) {
    out_off[p] = at;
    const int64_t a = page_off[p], n = page_off[p + 1] - a;
    uint8_t vi[10];
    const int nb = snpk::varint_len((uint64_t)n);
    uint64_t v = (uint64_t)n;
    for (int k = 0; k < nb; ++k, v >>= 7) vi[k] = (uint8_t)((v & 127u) | (k + 1 < nb ? 128u : 0u));
    put(vi, nb);
    for (int64_t b = 0; b < n; b += snpk::kBlock) {
      uint64_t size = 0;
      snpk::snappy_block(*S, in + a + b, (int)std::min<int64_t>(snpk::kBlock, n - b), tok.data(), slot.data(), &size);
      put(slot.data(), (int64_t)size);
    }
  }
  out_off[n_pages] = at;
  if (!fits) return fail(BQSR_ERR_INVALID_ARG, "bqsr_snappy_pages_host: the output does not fit (see out_off[n_pages])");
  return ok();
}

bqsr_status bqsr_parquet_pages_compress(bqsr_parquet_pages* enc, int32_t codec, void* stream, int64_t* comp_bytes) {
  if (!enc || !comp_bytes) return fail(BQSR_ERR_INVALID_ARG, "bqsr_parquet_pages_compress: bad arguments");
  if (codec != BQSR_PARQUET_CODEC_SNAPPY)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_parquet_pages_compress: the codec is BQSR_PARQUET_CODEC_SNAPPY");
  if (!enc->sized) return fail(BQSR_ERR_INVALID_ARG, "bqsr_parquet_pages_compress before bqsr_parquet_pages_size");
  enc->sized = false;  // (one compress per size call: the scratch is the next column's)
  g_pq_ms[PQ_EMIT] = 0.0;
  g_snappy_ms[SNAPPY_BLOCKS] = g_snappy_ms[SNAPPY_PACK] = 0.0;
  *comp_bytes = 0;
  enc->h_pages.clear();
  enc->comp_off.assign(1, 0);
  const pqk::Geo& G = enc->G;
  if (G.n_rows == 0) {
    enc->compressed = true;
    return ok();
  }
  HIP_TRY(hipSetDevice(enc->ctx->device));
  hipStream_t s = S(stream);
  uint8_t* out;
  bqsr_parquet_page* ptab;
  JOB_TRY(pq_emit_launch(enc, s, &out, &ptab));
  // the page table comes down first: the jobs are cut from it
  enc->h_pages.resize((size_t)G.n_pages);
  HIP_TRY(hipMemcpyAsync(enc->h_pages.data(), ptab, (size_t)G.n_pages * sizeof(bqsr_parquet_page),
                         hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  enc->clock.add(g_pq_ms[PQ_EMIT], PQ_EMIT_0, PQ_EMIT_1);
  SnappyPlan P;
  for (const bqsr_parquet_page& pg : enc->h_pages) {
    if (pg.offset < 0 || pg.bytes < 0 || pg.bytes > (int64_t)INT32_MAX || pg.offset + pg.bytes > enc->body_bytes)
      return fail(BQSR_ERR_DEVICE, "bqsr_parquet_pages_compress: a page outside the bodies");
    P.add_page((uint64_t)pg.offset, (uint64_t)pg.bytes);
  }
  std::vector<uint64_t> off;
  JOB_TRY(snappy_device(enc->ctx, out, P, s, *job_state<SnappyBufs>(enc->codec), off));
  enc->comp_off.resize((size_t)G.n_pages + 1);
  snappy_page_offsets(P, off, enc->comp_off.data());
  enc->compressed = true;
  *comp_bytes = enc->comp_off.back();
  return ok();
}

bqsr_status bqsr_parquet_pages_fetch(bqsr_parquet_pages* enc, uint8_t* comp, bqsr_parquet_page* pages,
                                     int64_t* comp_off, void* stream) {
  if (!enc || !comp_off) return fail(BQSR_ERR_INVALID_ARG, "bqsr_parquet_pages_fetch: bad arguments");
  if (!enc->compressed) return fail(BQSR_ERR_INVALID_ARG, "bqsr_parquet_pages_fetch before bqsr_parquet_pages_compress");
  const int64_t total = enc->comp_off.back();
  if ((total > 0 && !comp) || (!enc->h_pages.empty() && !pages))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_parquet_pages_fetch: bad arguments");
  enc->compressed = false;  // (one fetch per compress)
  if (total > 0) {
    HIP_TRY(hipSetDevice(enc->ctx->device));
    hipStream_t s = S(stream);
    HIP_TRY(hipMemcpyAsync(comp, job_state<SnappyBufs>(enc->codec)->packed.p, (size_t)total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  if (!enc->h_pages.empty()) memcpy(pages, enc->h_pages.data(), enc->h_pages.size() * sizeof(bqsr_parquet_page));
  memcpy(comp_off, enc->comp_off.data(), enc->comp_off.size() * sizeof(int64_t));
  return ok();
}

bqsr_status bqsr_parquet_pages_compress_times(double* snappy_ms, double* pack_ms) {
  if (snappy_ms) *snappy_ms = g_snappy_ms[SNAPPY_BLOCKS];
  if (pack_ms) *pack_ms = g_snappy_ms[SNAPPY_PACK];
  return BQSR_OK;
}

}  // extern "C"
