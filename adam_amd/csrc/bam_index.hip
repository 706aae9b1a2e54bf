// The .bai index of a BAM being written (SAM spec §5.2; include/adam_sam.h:
// bqsr_bam_index_*), built from what the BAM sink already holds on the device:
// where a record lies on the reference (bamo::bam_fields, the interval its bin
// field comes from) and where it lies in the record stream (the exclusive scan
// of bqsr_sam_bam_prepare).  `transform OUT.bam -bam_index` (transform._BamOut).
//
// One index object lives across the pieces and partitions of one output:
//
//   bai_rows      per piece, after its prepare: a lane per record appends a
//       row (refID, beg, end, FLAG & 4, stream offset) to a device array that
//       only grows.  Nothing is downloaded.
//   at the close, with the member table (stream start, file offset per BGZF
//   member) uploaded:
//   bai_locate    a lane per row: its virtual offsets u (the block_size word)
//       and v (one past its last byte) by binary search in the member table;
//       the order checks against the row before it and BAI's 2^29 limit, the
//       first offender by atomicMin on (ordinal << 8 | code); per reference
//       the counts of records with and without FLAG 0x4 and the largest end
//       (one atomic per wavefront where its 64 records share a reference), the
//       first u and the last v (written by the rows at a run's two ends).
//   bai_windows, bai_fill   the linear index: a 64-bit atomicMin per 16 kb
//       window a record touches, except the windows the lane before it (the
//       record before it in the file, with a smaller u) touches too; then per
//       reference a running maximum, which is "an empty window takes the value
//       of the window before it" because the filled values ascend.
//   bai_keys, (sort)   key = refID << 16 | reg2bin(beg, end), value = the row:
//       one stable rocprim::radix_sort_pairs over the key bits in use.
//   bai_heads, (scan), bai_emit, bai_ref_bins   a row starts a chunk when its
//       (refID, bin) differs from the row before it in sorted order, or the
//       chunk rule says so; one scan of (bin heads << 32 | chunk heads) numbers
//       both; the chunks' (u of the first row, v of the last), the bins' (key,
//       first chunk) and every reference's first bin are written compact.
//   Only those arrays, the windows and the per-reference words come back; the
//   host serialises them.
//
// HBM per record: 24 B row, 16 B (u, v), 16 B sort keys and 8 B sort values
// (double-buffered), 16 B heads and their scan: 80 B, plus rocprim's workspace;
// 16 B per chunk, 12 B per bin, 8 B per window.
//
// Included by bqsr_capi.cpp after bam_out.hip.

namespace baik {

constexpr int kThreads = 256;
constexpr uint32_t kMaxEnd = 1u << 29;  // BAI's limit: an end above it has no bin
constexpr uint32_t kPseudoBin = 37450;
enum : uint32_t { kBaiUnsorted = 1, kBaiLimit = 2, kBaiRef = 3 };  // error word: (row << 8) | code, the smallest wins

struct Row {
  int32_t ref;
  uint32_t beg;       // max(POS - 1, 0)
  uint32_t end;       // at least beg + 1; saturated at 2^32 - 1 (above kMaxEnd is refused anyway)
  uint32_t unmapped;  // FLAG & 4, the FLAG the record is written with
  uint64_t off;       // of the block_size word in the record stream (header bytes included)
};

struct RefWords {  // per reference; the entry after the last one counts refID -1
  unsigned long long mapped, unmapped, first_u, last_v;
  uint32_t max_end, pad;
};

struct RowsParams {
  bamo::BamParams P;  // of the piece's prepare: off is its scan
  Row* rows;          // where the piece's rows go
  uint64_t base;      // the stream offset of the piece's first byte
};

extern "C" __global__ void __launch_bounds__(kThreads) bai_rows(RowsParams A) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < A.P.n; i += (int64_t)gridDim.x * blockDim.x) {
    bamo::BamRec x;
    bamo::bam_fields(A.P, A.P.r0 + i, x);
    const int64_t beg = x.pos < 0 ? 0 : x.pos;
    const int64_t end = x.end < beg + 1 ? beg + 1 : x.end;
    A.rows[i] = Row{x.ref, (uint32_t)beg, (uint32_t)(end > 0xFFFFFFFFll ? 0xFFFFFFFFll : end), (uint32_t)(x.flag & 4),
                    A.base + A.P.off[i]};
  }
}

// The same row straight from a raw BAM record (`bam_index` on a file this project did not write, bam_windows.hip):
// buf holds the window's records, record i's block_size word at rec[i] and its end at rec[i + 1].  beg = max(pos, 0),
// end = pos + the CIGAR words' reference length over M D N = X (pos + 1 when that is 0), at least beg + 1.  A record
// whose name and CIGAR do not fit its block_size leaves (first + i) << 8 | 1 in *err, the smallest wins.
struct RawRecord {
  int32_t ref;
  uint32_t beg, end, flag;
  bool good;
};
__device__ __forceinline__ RawRecord raw_record(const uint8_t* b, uint64_t size) {
  const int64_t pos = (int32_t)bamk::rd32(b + 8);
  const uint32_t l_name = b[12], n_cig = bamk::rd16(b + 16);
  RawRecord r{(int32_t)bamk::rd32(b + 4), 0u, 1u, (uint32_t)bamk::rd16(b + 18), 36ull + l_name + 4ull * n_cig <= size};
  int64_t ref_len = 0;
  if (r.good) {
    const uint8_t* c = b + 36 + l_name;
    for (uint32_t k = 0; k < n_cig; ++k) {
      const uint32_t w = bamk::rd32(c + 4 * k), op = w & 15u;
      if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += w >> 4;
    }
  }
  const int64_t beg = pos < 0 ? 0 : pos;
  int64_t end = pos + (ref_len > 0 ? ref_len : 1);
  if (end < beg + 1) end = beg + 1;
  r.beg = (uint32_t)beg;
  r.end = (uint32_t)(end > 0xFFFFFFFFll ? 0xFFFFFFFFll : end);
  return r;
}

struct RawRowsParams {
  const uint8_t* buf;
  const uint64_t* rec;  // [n + 1]
  int64_t n;
  Row* rows;
  uint64_t base;        // the stream offset of buf[0]
  int64_t first;        // the ordinal of record 0 in the whole file
  unsigned long long* err;
};

extern "C" __global__ void __launch_bounds__(kThreads) bai_rows_raw(RawRowsParams A) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t o = A.rec[i];
    const RawRecord r = raw_record(A.buf + o, A.rec[i + 1] - o);
    if (!r.good) atomicMin(A.err, ((unsigned long long)(A.first + i) << 8) | 1ull);
    A.rows[i] = Row{r.ref, r.beg, r.end, r.flag & 4u, A.base + o};
  }
}

// mem: [2 (nm + 1)] (stream start, file offset) of every member, the EOF marker included, then the terminal entry.
// Position p lies in the last member whose start is not above it: among members of one start (an empty one
// before the next) that is the one that holds bytes, and for p = the stream's end it is the EOF marker.
__device__ __forceinline__ uint64_t virtual_offset(const uint64_t* mem, int64_t nm, uint64_t p) {
  int64_t a = 0, b = nm - 1;
  while (a < b) {
    const int64_t m = (a + b + 1) >> 1;
    if (mem[2 * m] <= p) a = m;
    else b = m - 1;
  }
  return (mem[2 * a + 1] << 16) | ((p - mem[2 * a]) & 0xFFFFu);
}

struct LocateParams {
  const Row* rows;
  int64_t n;
  uint64_t stream_end;
  const uint64_t* mem;
  int64_t nm;
  int32_t n_ref;
  uint64_t *u, *v;
  unsigned long long* err;
  RefWords* refs;  // [n_ref + 1]
};

// whole wavefronts take 64 consecutive rows, so the per-reference sums of a wavefront inside one reference
// (nearly all of them) leave as three atomics
extern "C" __global__ void __launch_bounds__(kThreads) bai_locate(LocateParams P) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < P.n; i0 += stride) {
    const int64_t i = i0 + lane;
    const bool live = i < P.n;
    Row r{-1, 0, 1, 0, 0};
    int slot = P.n_ref;
    bool good = false;  // a row whose reference has a slot
    if (live) {
      r = P.rows[i];
      uint32_t code = 0;
      if (r.ref >= P.n_ref) code = kBaiRef;
      if (!code && r.ref >= 0 && i > 0) {
        const Row q = P.rows[i - 1];
        if (q.ref < 0 || r.ref < q.ref || (r.ref == q.ref && r.beg < q.beg)) code = kBaiUnsorted;
      }
      if (!code && r.ref >= 0 && r.end > kMaxEnd) code = kBaiLimit;
      if (code) atomicMin(P.err, ((unsigned long long)i << 8) | code);
      good = r.ref < P.n_ref;
      const uint64_t u = virtual_offset(P.mem, P.nm, r.off);
      const uint64_t v = virtual_offset(P.mem, P.nm, i + 1 < P.n ? P.rows[i + 1].off : P.stream_end);
      P.u[i] = u;
      P.v[i] = v;
      if (good) {
        slot = r.ref < 0 ? P.n_ref : r.ref;
        if (i == 0 || P.rows[i - 1].ref != r.ref) P.refs[slot].first_u = u;
        if (i + 1 == P.n || P.rows[i + 1].ref != r.ref) P.refs[slot].last_v = v;
      }
    }
    const int slot0 = __shfl(slot, 0);
    if (__all(!live || (good && slot == slot0))) {
      const unsigned long long nu = __popcll(__ballot(live && r.unmapped)), na = __popcll(__ballot(live));
      uint32_t me = live ? r.end : 0u;
      for (int d = 32; d; d >>= 1) me = max(me, (uint32_t)__shfl_xor((int)me, d));
      if (lane == 0) {  // (lane 0 is live, so slot0 is a reference's)
        if (na - nu) atomicAdd(&P.refs[slot0].mapped, na - nu);
        if (nu) atomicAdd(&P.refs[slot0].unmapped, nu);
        atomicMax(&P.refs[slot0].max_end, me);
      }
    } else if (live && good) {
      atomicAdd(r.unmapped ? &P.refs[slot].unmapped : &P.refs[slot].mapped, 1ull);
      atomicMax(&P.refs[slot].max_end, r.end);
    }
  }
}

// rows [0, np) are the placed ones, in (refID, beg) order (bai_locate checked it), so their u ascend: the
// smallest u of a window is that of the first row that touches it, and a row need not touch a window the row
// before it touches: the lane before holds that row, so a lane leaves those windows out.  (Measured on 2M reads
// of 100 bases, profiles/bam_index_2m.json: 0.033 ms for this stage, 0.33 ms with every lane touching all of its
// windows; that form is not kept.)  Every end is <= kMaxEnd here.
extern "C" __global__ void __launch_bounds__(kThreads) bai_windows(const Row* rows, int64_t np, const uint64_t* u,
                                                                  const uint64_t* lin_off, unsigned long long* win) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < np; i0 += stride) {
    const int64_t i = i0 + lane;
    const bool live = i < np;
    int ref = -1, lo = 0, hi = -1;
    if (live) {
      const Row r = rows[i];
      ref = r.ref;
      lo = (int)(r.beg >> 14);
      hi = (int)((r.end - 1) >> 14);
    }
    const int pref = __shfl_up(ref, 1), phi = __shfl_up(hi, 1);
    if (lane > 0 && pref == ref && phi + 1 > lo) lo = phi + 1;
    if (live) {
      const unsigned long long ui = u[i];
      unsigned long long* w = win + lin_off[ref];
      for (int k = lo; k <= hi; ++k) atomicMin(w + k, ui);
    }
  }
}

// a block per reference: untouched windows (~0) become 0, then every window the maximum of those up to it
extern "C" __global__ void __launch_bounds__(kThreads) bai_fill(const uint64_t* lin_off, int32_t n_ref,
                                                               unsigned long long* win) {
  __shared__ unsigned long long wave_max[kThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int32_t ref = blockIdx.x; ref < n_ref; ref += gridDim.x) {
    const uint64_t a = lin_off[ref], b = lin_off[ref + 1];
    unsigned long long carry = 0;
    for (uint64_t base = a; base < b; base += kThreads) {
      const uint64_t k = base + threadIdx.x;
      unsigned long long x = k < b ? win[k] : 0ull;
      if (x == ~0ull) x = 0;
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(x, d);
        if (lane >= d && t > x) x = t;
      }
      if (lane == 63) wave_max[wave] = x;
      __syncthreads();
      unsigned long long all = carry;
      for (int q = 0; q < kThreads / 64; ++q) {
        if (q < wave && wave_max[q] > x) x = wave_max[q];
        if (wave_max[q] > all) all = wave_max[q];
      }
      if (carry > x) x = carry;
      if (k < b) win[k] = x;
      carry = all;
      __syncthreads();
    }
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) bai_keys(const Row* rows, int64_t np, uint64_t* key,
                                                               uint32_t* val) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < np; j += (int64_t)gridDim.x * blockDim.x) {
    const Row r = rows[j];
    key[j] = ((uint64_t)(uint32_t)r.ref << 16) | bamo::reg2bin((int64_t)r.beg, (int64_t)r.end);
    val[j] = (uint32_t)j;
  }
}

// sorted position j: bin head << 32 | chunk head.  Inside one (refID, bin) the rows are in file order; a row
// joins the chunk before it when that chunk ends in or after the member the row starts in.
extern "C" __global__ void __launch_bounds__(kThreads) bai_heads(const uint64_t* key, const uint32_t* val, int64_t np,
                                                                const uint64_t* u, const uint64_t* v, uint64_t* head) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < np; j += (int64_t)gridDim.x * blockDim.x) {
    const bool nb = j == 0 || key[j] != key[j - 1];
    const bool nc = nb || !((v[val[j - 1]] >> 16) >= (u[val[j]] >> 16));
    head[j] = ((uint64_t)nb << 32) | (uint64_t)nc;
  }
}

struct EmitParams {
  const uint64_t* key;
  const uint32_t* val;
  const uint64_t *head, *id;  // id: the inclusive scan of head
  const uint64_t *u, *v;
  int64_t np;
  uint64_t *cbeg, *cend;  // [n_chunks]
  uint64_t* bkey;         // [n_bins]
  uint32_t* bchunk;       // [n_bins + 1] a bin's first chunk
};

extern "C" __global__ void __launch_bounds__(kThreads) bai_emit(EmitParams P) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < P.np; j += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t h = P.head[j], w = P.id[j];
    const uint32_t c = (uint32_t)w - 1, b = (uint32_t)(w >> 32) - 1;
    const uint32_t r = P.val[j];
    if (h & 1u) P.cbeg[c] = P.u[r];
    const bool last = j + 1 == P.np;
    if (last || (P.head[j + 1] & 1u)) P.cend[c] = P.v[r];
    if (h >> 32) {
      P.bkey[b] = P.key[j];
      P.bchunk[b] = c;
    }
    if (last) P.bchunk[b + 1] = c + 1;
  }
}

// ref_bin[r]: the first bin of reference r or a later one, r = 0 .. n_ref
extern "C" __global__ void __launch_bounds__(kThreads) bai_ref_bins(const uint64_t* bkey, int64_t n_bins, int32_t n_ref,
                                                                   uint32_t* ref_bin) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r <= n_ref; r += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = 0, b = n_bins;
    while (a < b) {
      const int64_t m = (a + b) >> 1;
      if (bkey[m] < ((uint64_t)r << 16)) a = m + 1;
      else b = m;
    }
    ref_bin[r] = (uint32_t)a;
  }
}

}  // namespace baik

// the stages of an index (transform.BAM_INDEX_KERNELS; the last is the host's), and the clock's marks
enum { BAI_ROWS, BAI_LOCATE, BAI_WINDOWS, BAI_SORT, BAI_CHUNKS, BAI_SERIALIZE_HOST, BAI_STAGES };
enum { BAI_ROWS_0, BAI_ROWS_1, BAI_LOCATE_0, BAI_LOCATE_1, BAI_WINDOWS_0, BAI_SORT_0, BAI_CHUNKS_0, BAI_CHUNKS_1,
       BAI_MARKS };

struct bqsr_bam_index {
  bqsr_context* ctx = nullptr;
  bool on_device = false;  // a call has selected the context's device: destroy frees there
  int32_t n_ref = 0;
  baik::Row* rows = nullptr;  // grown with its contents kept
  int64_t cap_rows = 0, n_rows = 0;
  uint64_t stream_end = 0;  // one past the last added piece
  bool has_members = false, finished = false, rows_timed = true;
  int64_t nm = 0;
  DevBuf mem, u, v, err, refs, lin_off, win, key_a, key_b, val_a, val_b, head, id, cbeg, cend, bkey, bchunk, ref_bin,
      temp;
  StageClock<BAI_MARKS> clock;
  double ms[BAI_STAGES] = {0, 0, 0, 0, 0, 0};
  bqsr_bam_index_sizes sizes{0, 0, 0, 0, 0, 0};
  std::string bytes;
  ~bqsr_bam_index() {
    if (rows) (void)hipFree(rows);
  }
};

namespace {

// the rows kernel of the add before: its marks are read once it is over, without a wait inside the add itself
void bai_rows_time(bqsr_bam_index& X) {
  if (X.rows_timed) return;
  if (hipEventSynchronize(X.clock.ev[BAI_ROWS_1]) == hipSuccess) X.clock.add(X.ms[BAI_ROWS], BAI_ROWS_0, BAI_ROWS_1);
  X.rows_timed = true;
}

template <class T>
void bai_put(std::string& o, T v) {
  o.append((const char*)&v, sizeof v);
}

// room for n more rows: grown with what it holds (a new array, a copy, the old one freed after it)
bqsr_status bai_rows_reserve(bqsr_bam_index& X, int64_t n, hipStream_t st) {
  if (X.cap_rows < X.n_rows + n) {
    const int64_t cap = std::max<int64_t>(X.n_rows + n, 2 * X.cap_rows);
    baik::Row* p = nullptr;
    if (hipMalloc((void**)&p, (size_t)cap * sizeof(baik::Row)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(BQSR_ERR_UNSUPPORTED, "BAM index: the rows of the whole output stay resident on the device and do "
                                        "not fit: " + std::to_string((size_t)cap * sizeof(baik::Row)) + " bytes");
    }
    hipError_t e = hipSuccess;
    if (X.n_rows > 0) {
      e = hipMemcpyAsync(p, X.rows, (size_t)X.n_rows * sizeof(baik::Row), hipMemcpyDeviceToDevice, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) {
      (void)hipFree(p);
      return fail(BQSR_ERR_DEVICE, std::string("bqsr_bam_index_add: ") + hipGetErrorString(e));
    }
    if (X.rows) (void)hipFree(X.rows);
    X.rows = p;
    X.cap_rows = cap;
  }
  return BQSR_OK;
}

}  // namespace

extern "C" {

bqsr_status bqsr_bam_index_create(bqsr_context* ctx, int32_t n_ref, bqsr_bam_index** out) {
  if (!ctx || !out || n_ref < 0) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_create: bad arguments");
  *out = new (std::nothrow) bqsr_bam_index;
  if (!*out) return fail(BQSR_ERR_DEVICE, "bqsr_bam_index_create: out of host memory");
  (*out)->ctx = ctx;
  (*out)->n_ref = n_ref;
  return ok();
}

void bqsr_bam_index_destroy(bqsr_bam_index* x) {
  if (!x) return;
  if (x->on_device) (void)hipSetDevice(x->ctx->device);
  delete x;
}

bqsr_status bqsr_bam_index_add(bqsr_bam_index* x, bqsr_sam* s, int64_t stream_base, void* stream) {
  if (!x || !s || stream_base < 0) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_add: bad arguments");
  bqsr_bam_index& X = *x;
  BamBufs* Ap = (BamBufs*)s->bam.get();
  if (!Ap || !Ap->prepared || Ap->text != s->d_text || Ap->spans != s->line_span)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_add before bqsr_sam_bam_prepare of the piece");
  if (X.has_members || X.finished) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_add after the member table");
  if ((uint64_t)stream_base < X.stream_end)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_add: a piece that starts before the end of the one before it");
  BamBufs& A = *Ap;
  if (X.n_rows + A.n > (int64_t)0xFFFFFFFFll)
    return fail(BQSR_ERR_UNSUPPORTED, "BAM index: more than 2^32 - 1 records in one index");
  HIP_TRY(hipSetDevice(X.ctx->device));
  X.on_device = true;
  hipStream_t st = S(stream);
  bai_rows_time(X);
  JOB_TRY(bai_rows_reserve(X, A.n, st));
  if (A.n > 0) {
    baik::RowsParams R{bam_params(s, A), X.rows + X.n_rows, (uint64_t)stream_base};
    HIP_TRY(X.clock.mark(BAI_ROWS_0, st));
    JOB_TRY(launch(baik::bai_rows, sam_grid(A.n, baik::kThreads, X.ctx->n_cu * 8), baik::kThreads, st, R));
    HIP_TRY(X.clock.mark(BAI_ROWS_1, st));
    X.rows_timed = false;
  }
  X.n_rows += A.n;
  X.stream_end = (uint64_t)stream_base + (uint64_t)A.total;
  return ok();
}

bqsr_status bqsr_bam_index_set_members(bqsr_bam_index* x, const uint64_t* members, int64_t n_members, void* stream) {
  if (!x || !members || n_members < 1) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_set_members: bad arguments");
  bqsr_bam_index& X = *x;
  if (X.finished) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_set_members after bqsr_bam_index_finish");
  // [n_members] members and the terminal entry: the stream from 0 on without a gap, no member above what BSIZE
  // and the 16 offset bits hold, file offsets ascending and below 2^48, the stream's end where the pieces ended
  bool good = members[0] == 0;
  for (int64_t m = 0; good && m < n_members; ++m)
    good = members[2 * m] <= members[2 * m + 2] && members[2 * m + 2] - members[2 * m] <= 65536 &&
           members[2 * m + 1] < members[2 * m + 3] && members[2 * m + 3] < (1ull << 48);
  if (good && X.n_rows > 0) good = members[2 * n_members] == X.stream_end;
  if (!good)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_set_members: not the member table of the stream that was added");
  HIP_TRY(hipSetDevice(X.ctx->device));
  X.on_device = true;
  hipStream_t st = S(stream);
  uint64_t* d;
  JOB_TRY(dev_need(X.mem, &d, (size_t)(2 * (n_members + 1)), "BAM index", "member table"));
  HIP_TRY(hipMemcpyAsync(d, members, (size_t)(2 * (n_members + 1)) * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  X.nm = n_members;
  if (X.n_rows == 0) X.stream_end = members[2 * n_members];
  X.has_members = true;
  return ok();
}

bqsr_status bqsr_bam_index_finish(bqsr_bam_index* x, void* stream) {
  using namespace baik;
  if (!x) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_finish: bad arguments");
  bqsr_bam_index& X = *x;
  if (!X.has_members) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_finish before bqsr_bam_index_set_members");
  if (X.finished) return ok();
  HIP_TRY(hipSetDevice(X.ctx->device));
  hipStream_t s = S(stream);
  bai_rows_time(X);
  bqsr_status e;
  auto need = [](DevBuf& b, auto** p, size_t count, const char* what) {
    return dev_need(b, p, count, "BAM index", what);
  };
  auto prim = [&](auto&& call) { return dev_prim(X.temp, "BAM index", call); };
  auto grid = [&](int64_t items) { return sam_grid(items, kThreads, X.ctx->n_cu * 8); };
  const int64_t n = X.n_rows;
  const size_t N = (size_t)n, NR = (size_t)X.n_ref;
  // ---- locate ----
  std::vector<RefWords> refs(NR + 1, RefWords{0, 0, 0, 0, 0, 0});
  uint64_t *u = nullptr, *v = nullptr;
  if (n > 0) {
    unsigned long long* err;
    RefWords* d_refs;
    if ((e = need(X.u, &u, N, "records")) || (e = need(X.v, &v, N, "records")) ||
        (e = need(X.err, &err, 1, "status word")) || (e = need(X.refs, &d_refs, NR + 1, "references")))
      return e;
    HIP_TRY(hipMemsetAsync(err, 0xFF, 8, s));
    HIP_TRY(hipMemsetAsync(d_refs, 0, (NR + 1) * sizeof(RefWords), s));
    LocateParams L{X.rows, n, X.stream_end, (const uint64_t*)X.mem.p, X.nm, X.n_ref, u, v, err, d_refs};
    HIP_TRY(X.clock.mark(BAI_LOCATE_0, s));
    JOB_TRY(launch(bai_locate, grid(n), kThreads, s, L));
    HIP_TRY(X.clock.mark(BAI_LOCATE_1, s));
    unsigned long long ew = ~0ull;
    HIP_TRY(hipMemcpyAsync(&ew, err, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(refs.data(), d_refs, (NR + 1) * sizeof(RefWords), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    X.clock.add(X.ms[BAI_LOCATE], BAI_LOCATE_0, BAI_LOCATE_1);
    if (ew != ~0ull) {
      const uint32_t code = (uint32_t)(ew & 0xFF);
      const int64_t read = (int64_t)(ew >> 8);
      const std::string who = "BAM index: read " + std::to_string(read) + " of the output: ";
      if (code == kBaiUnsorted)
        return fail(BQSR_ERR_UNSORTED, who + "the output is not in coordinate order (among the reads with an RNAME the "
                                             "reference index or the start decreases, or one follows a read without)",
                    read);
      if (code == kBaiLimit)
        return fail(BQSR_ERR_UNSUPPORTED, who + "it ends above position 2^29, the limit of a .bai index", read);
      return fail(BQSR_ERR_INVALID_ARG, who + "a reference index outside the index's references", read);
    }
  }
  const int64_t n_no_coor = (int64_t)(refs[NR].mapped + refs[NR].unmapped);
  const int64_t np = n - n_no_coor;  // the placed rows come first
  // ---- windows ----
  std::vector<uint64_t> lin_off(NR + 1, 0);
  for (size_t r = 0; r < NR; ++r) {
    const bool any = refs[r].mapped + refs[r].unmapped > 0;
    lin_off[r + 1] = lin_off[r] + (any ? 1 + ((refs[r].max_end - 1) >> 14) : 0);
  }
  const size_t W = (size_t)lin_off[NR];
  std::vector<uint64_t> win(W), cbeg, cend, bkey;
  std::vector<uint32_t> bchunk(1, 0), ref_bin(NR + 1, 0);
  if (np > 0) {
    const size_t NP = (size_t)np;
    uint64_t *d_lin, *key_a, *key_b, *head, *id;
    unsigned long long* d_win;
    uint32_t *val_a, *val_b;
    if ((e = need(X.lin_off, &d_lin, NR + 1, "references")) || (e = need(X.win, &d_win, W, "windows")) ||
        (e = need(X.key_a, &key_a, NP, "records")) || (e = need(X.key_b, &key_b, NP, "records")) ||
        (e = need(X.val_a, &val_a, NP, "records")) || (e = need(X.val_b, &val_b, NP, "records")) ||
        (e = need(X.head, &head, NP, "records")) || (e = need(X.id, &id, NP, "records")))
      return e;
    HIP_TRY(hipMemcpyAsync(d_lin, lin_off.data(), (NR + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(X.clock.mark(BAI_WINDOWS_0, s));
    HIP_TRY(hipMemsetAsync(d_win, 0xFF, W * 8, s));
    JOB_TRY(launch(bai_windows, grid(np), kThreads, s, X.rows, np, u, d_lin, d_win));
    JOB_TRY(launch(bai_fill, sam_grid(X.n_ref, 1, X.ctx->n_cu * 8), kThreads, s, d_lin, X.n_ref, d_win));
    HIP_TRY(X.clock.mark(BAI_SORT_0, s));
    // ---- sort by (refID, bin) ----
    int max_ref = 0;
    for (size_t r = 0; r < NR; ++r)
      if (refs[r].mapped + refs[r].unmapped > 0) max_ref = (int)r;
    const unsigned key_bits = 16u + (unsigned)bits_of((uint64_t)max_ref);
    JOB_TRY(launch(bai_keys, grid(np), kThreads, s, X.rows, np, key_a, val_a));
    if ((e = prim([&](void* t, size_t& b) {
           return rocprim::radix_sort_pairs(t, b, key_a, key_b, val_a, val_b, NP, 0, key_bits, s);
         })))
      return e;
    HIP_TRY(X.clock.mark(BAI_CHUNKS_0, s));
    // ---- chunks and bins ----
    JOB_TRY(launch(bai_heads, grid(np), kThreads, s, key_b, val_b, np, u, v, head));
    if ((e = prim([&](void* t, size_t& b) {
           return rocprim::inclusive_scan(t, b, head, id, NP, rocprim::plus<uint64_t>(), s);
         })))
      return e;
    uint64_t totals = 0;
    HIP_TRY(hipMemcpyAsync(&totals, id + (np - 1), 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const size_t NC = (size_t)(uint32_t)totals, NB = (size_t)(totals >> 32);
    uint64_t *d_cbeg, *d_cend, *d_bkey;
    uint32_t *d_bchunk, *d_ref_bin;
    if ((e = need(X.cbeg, &d_cbeg, NC, "chunks")) || (e = need(X.cend, &d_cend, NC, "chunks")) ||
        (e = need(X.bkey, &d_bkey, NB, "bins")) || (e = need(X.bchunk, &d_bchunk, NB + 1, "bins")) ||
        (e = need(X.ref_bin, &d_ref_bin, NR + 1, "references")))
      return e;
    EmitParams E{key_b, val_b, head, id, u, v, np, d_cbeg, d_cend, d_bkey, d_bchunk};
    JOB_TRY(launch(bai_emit, grid(np), kThreads, s, E));
    JOB_TRY(launch(bai_ref_bins, grid((int64_t)NR + 1), kThreads, s, d_bkey, (int64_t)NB, X.n_ref, d_ref_bin));
    HIP_TRY(X.clock.mark(BAI_CHUNKS_1, s));
    cbeg.resize(NC);
    cend.resize(NC);
    bkey.resize(NB);
    bchunk.resize(NB + 1);
    HIP_TRY(hipMemcpyAsync(cbeg.data(), d_cbeg, NC * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cend.data(), d_cend, NC * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(bkey.data(), d_bkey, NB * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(bchunk.data(), d_bchunk, (NB + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(ref_bin.data(), d_ref_bin, (NR + 1) * 4, hipMemcpyDeviceToHost, s));
    if (W) HIP_TRY(hipMemcpyAsync(win.data(), d_win, W * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    X.clock.add(X.ms[BAI_WINDOWS], BAI_WINDOWS_0, BAI_SORT_0);
    X.clock.add(X.ms[BAI_SORT], BAI_SORT_0, BAI_CHUNKS_0);
    X.clock.add(X.ms[BAI_CHUNKS], BAI_CHUNKS_0, BAI_CHUNKS_1);
  }
  // ---- the file (SAM spec §5.2), on the host ----
  const auto t0 = std::chrono::steady_clock::now();
  std::string& o = X.bytes;
  o.assign("BAI\1", 4);
  o.reserve(16 + 16 * cbeg.size() + 8 * bkey.size() + 8 * W + 56 * NR);
  bai_put<int32_t>(o, X.n_ref);
  for (size_t r = 0; r < NR; ++r) {
    if (refs[r].mapped + refs[r].unmapped == 0) {
      bai_put<int32_t>(o, 0);
      bai_put<int32_t>(o, 0);
      continue;
    }
    bai_put<int32_t>(o, (int32_t)(ref_bin[r + 1] - ref_bin[r]) + 1);
    for (uint32_t b = ref_bin[r]; b < ref_bin[r + 1]; ++b) {
      bai_put<uint32_t>(o, (uint32_t)(bkey[b] & 0xFFFFu));
      bai_put<int32_t>(o, (int32_t)(bchunk[b + 1] - bchunk[b]));
      for (uint32_t c = bchunk[b]; c < bchunk[b + 1]; ++c) {
        bai_put<uint64_t>(o, cbeg[c]);
        bai_put<uint64_t>(o, cend[c]);
      }
    }
    bai_put<uint32_t>(o, kPseudoBin);
    bai_put<int32_t>(o, 2);
    bai_put<uint64_t>(o, refs[r].first_u);
    bai_put<uint64_t>(o, refs[r].last_v);
    bai_put<uint64_t>(o, refs[r].mapped);
    bai_put<uint64_t>(o, refs[r].unmapped);
    bai_put<int32_t>(o, (int32_t)(lin_off[r + 1] - lin_off[r]));
    o.append((const char*)(win.data() + lin_off[r]), (size_t)(lin_off[r + 1] - lin_off[r]) * 8);
  }
  bai_put<uint64_t>(o, (uint64_t)n_no_coor);
  X.ms[BAI_SERIALIZE_HOST] =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  size_t dev = (size_t)X.cap_rows * sizeof(Row);
  for (const DevBuf* b : {&X.mem, &X.u, &X.v, &X.err, &X.refs, &X.lin_off, &X.win, &X.key_a, &X.key_b, &X.val_a,
                          &X.val_b, &X.head, &X.id, &X.cbeg, &X.cend, &X.bkey, &X.bchunk, &X.ref_bin, &X.temp})
    dev += b->cap;
  X.sizes = bqsr_bam_index_sizes{n, (int64_t)cbeg.size(), (int64_t)bkey.size(), (int64_t)W, (int64_t)o.size(),
                                 (int64_t)dev};
  X.finished = true;
  return ok();
}

bqsr_status bqsr_bam_index_size(const bqsr_bam_index* x, bqsr_bam_index_sizes* out) {
  if (!x || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_size: bad arguments");
  if (!x->finished) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_size before bqsr_bam_index_finish");
  *out = x->sizes;
  return ok();
}

bqsr_status bqsr_bam_index_bytes(const bqsr_bam_index* x, uint8_t* dst, int64_t cap) {
  if (!x || !dst || cap < 0) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_bytes: bad arguments");
  if (!x->finished) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_bytes before bqsr_bam_index_finish");
  if ((size_t)cap < x->bytes.size())
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_bytes: the index does not fit (see bqsr_bam_index_size)");
  memcpy(dst, x->bytes.data(), x->bytes.size());
  return ok();
}

bqsr_status bqsr_bam_index_kernel_times(const bqsr_bam_index* x, double* ms6) {
  if (!x || !ms6) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_kernel_times: bad arguments");
  for (int k = 0; k < BAI_STAGES; ++k) ms6[k] = x->ms[k];
  return BQSR_OK;
}

}  // extern "C"
