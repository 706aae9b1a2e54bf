// A BAM read in windows (include/adam_sam.h: bqsr_bam_reader_*): a window is a
// run of whole BGZF members of a mapped file, inflated on the device by
// bgzf_inflate_runs' kernels; the offsets of its complete records are found
// from a known first-record offset by the guess / check / write chain of
// bgzf_inflate.hip in its window form (the start is given, the last walk may
// leave the window).  Device memory is bounded by the window, not by the file.
//
//   `python -m adam_amd.bam_index IN.bam`: every window's records leave a row
//       each in a bqsr_bam_index (bai_rows_raw, bam_index.hip), the member
//       table is the file's own, bai_locate onward is unchanged.
//   `-region` (inputs.SamInput): per chunk of the index the windows from u's
//       member on; region_filter keeps the records that overlap the region,
//       a scan and region_copy compact them into one buffer that lives across
//       windows; that buffer goes through bam_lines_text / sam_parse_device.
//
// Included by bqsr_capi.cpp after bam_index.hip.

namespace bamw {

constexpr int kThreads = 256;
constexpr int kCountShift = 38;  // a scan word: kept records << 38 | kept bytes (a window is at most 2^31 bytes)
constexpr uint64_t kBytesMask = (1ull << kCountShift) - 1;

struct WindowChain {
  bgzfk::ChainParams C;  // body: the first record's offset in the window; m: the window's length
  int64_t* stop;         // where the chain ended: m, or the record the window cuts (starts at m until a walk says)
};

// a record at q that the window cuts: its block_size word, or what that word promises, lies past the end
__device__ __forceinline__ bool cut_record(const bgzfk::ChainParams& C, int64_t q) {
  if (q >= C.m) return false;
  if (q + 4 > C.m) return true;
  const int64_t bs = bgzfk::ld32(C.u + q);
  return bs >= 32 && q + 4 + bs > C.m;
}

// pass 1 (bam_chain_guess with the window's two rules): block 0's start is the given one; a start is also
// plausible when the record after it is the one the window cuts; a walk ends at the first record it cannot finish
extern "C" __global__ void bam_window_guess(WindowChain W) {
  const bgzfk::ChainParams& C = W.C;
  const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (b >= C.n_blk) return;
  int64_t lo, hi;
  bgzfk::blk_range(C, b, lo, hi);
  int64_t g = -1;
  if (lo < hi) {
    if (C.body >= C.blks[b].dst && C.body < hi) {
      g = C.body;
    } else {
      for (int64_t p = lo; p < hi; ++p) {
        if (!bgzfk::rec_plausible(C.u, p, C.m, C.n_ref)) continue;
        const int64_t q = p + 4 + bgzfk::ld32(C.u + p);
        if (q == C.m || bgzfk::rec_plausible(C.u, q, C.m, C.n_ref) || cut_record(C, q)) {
          g = p;
          break;
        }
      }
    }
  }
  uint64_t n = 0;
  int64_t p = g;
  if (g >= 0) {
    while (p < hi) {
      if (p + 4 > C.m) break;
      const int64_t bs = bgzfk::ld32(C.u + p);
      if (bs < 32) { atomicOr(C.bad, 1); break; }
      if (p + 4 + bs > C.m) break;
      p += 4 + bs;
      ++n;
    }
  }
  C.guess[b] = g;
  C.exit[b] = p;
  C.count[b] = n;
}

// pass 2 (bam_chain_check): a walk that ends on m or on the cut record ends the chain and names the stop
extern "C" __global__ void bam_window_check(WindowChain W) {
  const bgzfk::ChainParams& C = W.C;
  const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (b >= C.n_blk) return;
  int64_t lo, hi;
  bgzfk::blk_range(C, b, lo, hi);
  const bool has_body = lo < hi && C.body >= C.blks[b].dst && C.body < hi;
  if (C.guess[b] < 0) {
    if (has_body) atomicOr(C.bad, 1);
    return;
  }
  const int64_t e = C.exit[b];
  if (e > C.m) { atomicOr(C.bad, 1); return; }
  if (e == C.m || cut_record(C, e)) {
    for (int64_t k = b + 1; k < C.n_blk; ++k)
      if (C.guess[k] >= 0) { atomicOr(C.bad, 1); break; }
    *W.stop = e;  // (one block of a good chain gets here)
    return;
  }
  if (e < hi) { atomicOr(C.bad, 1); return; }  // (a walk leaves its block unless it ends the chain)
  for (int64_t k = b + 1; k < C.n_blk; ++k) {
    int64_t l2, h2;
    bgzfk::blk_range(C, k, l2, h2);
    if (e >= h2) {
      if (C.guess[k] >= 0) { atomicOr(C.bad, 1); return; }
      continue;
    }
    if (C.guess[k] != e) atomicOr(C.bad, 1);
    return;
  }
  atomicOr(C.bad, 1);
}

// pass 3 (bam_chain_write): the complete records' offsets
extern "C" __global__ void bam_window_write(WindowChain W) {
  const bgzfk::ChainParams& C = W.C;
  const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (b >= C.n_blk) return;
  int64_t lo, hi;
  bgzfk::blk_range(C, b, lo, hi);
  int64_t p = C.guess[b];
  if (p < 0) return;
  const int64_t stop = *W.stop;
  uint64_t i = C.base[b];
  while (p < hi && p < stop) {
    C.rec[i++] = (uint64_t)(p - C.body);
    p += 4 + bgzfk::ld32(C.u + p);
  }
}

// ---- a region's records ----
struct FilterParams {
  const uint8_t* buf;   // the window's records
  const uint64_t* rec;  // [n + 1]
  int64_t n;
  uint64_t base;        // the stream offset of buf[0]
  uint64_t limit;       // the stream offset of the chunk's v: a record at or past it is not taken
  int32_t rid;
  uint32_t rbeg, rend;
  uint64_t* len;        // [n] kept: 1 << kCountShift | its bytes; else 0
  unsigned long long* stop;  // the first record that ends the chunk (i << 1 | 1) or the region (i << 1); ~0 none
  unsigned long long* err;   // a malformed record, as bai_rows_raw leaves it
  int64_t first;
};

// a lane per record: kept when refID == rid, beg < region end, end > region beg (the index's interval, so a
// placed read with FLAG 0x4 is kept).  In a sorted file nothing after a record of a later reference (or
// without one), or with beg >= region end, overlaps the region: the first such record ends the read.
extern "C" __global__ void __launch_bounds__(kThreads) region_filter(FilterParams A) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t o = A.rec[i], size = A.rec[i + 1] - o;
    const baik::RawRecord r = baik::raw_record(A.buf + o, size);
    const bool past = A.base + o >= A.limit;
    if (!r.good && !past) atomicMin(A.err, ((unsigned long long)(A.first + i) << 8) | 1ull);  // (only a record the read takes)
    const bool later = r.ref < 0 || r.ref > A.rid || (r.ref == A.rid && r.beg >= A.rend);
    if (later) atomicMin(A.stop, (unsigned long long)i << 1);
    else if (past) atomicMin(A.stop, ((unsigned long long)i << 1) | 1ull);
    const bool keep = !past && r.ref == A.rid && r.beg < A.rend && r.end > A.rbeg;
    A.len[i] = keep ? (1ull << kCountShift) | size : 0ull;
  }
}

struct CopyParams {
  const uint8_t* buf;
  const uint64_t* rec;
  const uint64_t* len;  // [n]
  const uint64_t* off;  // [n + 1] its exclusive scan
  int64_t n;
  uint8_t* out;         // the kept bytes of this window go to out[0 ..)
  uint64_t* out_rec;    // and their offsets to out_rec[0 ..)
  uint64_t out_base;    // the kept bytes before this window
};

// A wavefront takes 64 consecutive records: their kept bytes are one contiguous range of the output, which the
// lanes store 64 bytes a step; a byte's record is the last of the 64 whose scanned offset is not above it (a
// binary search through the lanes' registers).
extern "C" __global__ void __launch_bounds__(kThreads) region_copy(CopyParams A) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < A.n; i0 += stride) {
    const int64_t i = i0 + lane;
    const bool live = i < A.n;
    const unsigned long long w = A.off[live ? i : A.n];
    const unsigned long long my_off = w & kBytesMask;
    const unsigned long long my_src = live ? A.rec[i] : 0ull;
    if (live && A.len[i]) A.out_rec[w >> kCountShift] = A.out_base + my_off;
    const int64_t last = i0 + 64 < A.n ? i0 + 64 : A.n;
    const unsigned long long b0 = A.off[i0] & kBytesMask, b1 = A.off[last] & kBytesMask;
    for (unsigned long long j0 = b0; j0 < b1; j0 += 64) {  // (uniform over the wavefront: every lane shuffles)
      const unsigned long long j = j0 + lane;
      int r = 0;
      for (int d = 32; d; d >>= 1) {
        const unsigned long long o = __shfl(my_off, r + d);
        if (o <= j) r += d;
      }
      const unsigned long long ro = __shfl(my_off, r), rs = __shfl(my_src, r);
      if (j < b1) A.out[j] = A.buf[rs + (j - ro)];
    }
  }
}

}  // namespace bamw

struct bqsr_bam_reader {
  bqsr_context* ctx = nullptr;
  const uint8_t* data = nullptr;
  int64_t n = 0, piece = 0;
  std::vector<BgzfBlk> blks;       // src, csize, dst, isize of every member
  std::vector<int64_t> file_off;   // [nb + 1] where each member starts in the file
  int64_t m = 0;                   // the inflated stream's length
  BamHead BH;
  SamHeader H;
  std::string hdr;
  int64_t p = 0;                   // the stream offset of the next record
  // the current window
  std::vector<void*> win;          // its device allocations
  uint8_t* d_raw = nullptr;
  uint64_t* d_rec = nullptr;       // [nr + 1] from `start`
  int64_t b0 = 0, b1 = 0, m_w = 0, start = 0, stop = 0, nr = 0, first = 0;
  bool have_window = false;
  // the kept records of a region read
  uint8_t* keep = nullptr;
  uint64_t* keep_rec = nullptr;
  int64_t keep_cap = 0, keep_bytes = 0, keep_rec_cap = 0, keep_n = 0;
  bqsr_bam_reader_stats st{};
  StageClock<2> clock;
  void drop_window() {
    for (void* q : win) (void)hipFree(q);
    win.clear();
    d_raw = nullptr;
    d_rec = nullptr;
    have_window = false;
  }
  ~bqsr_bam_reader() {
    drop_window();
    if (keep) (void)hipFree(keep);
    if (keep_rec) (void)hipFree(keep_rec);
  }
};

namespace {

// members [b0, b1) inflated into R.d_raw (m_w bytes, 64 zero bytes after them): the device kernels, and for a
// member they decline the host's inflate (which reports a damaged member)
bqsr_status window_inflate(bqsr_bam_reader& R, int64_t b0, int64_t b1, hipStream_t s, bgzfk::Blk** d_blk) {
  R.drop_window();
  const int64_t dst0 = R.blks[(size_t)b0].dst, c0 = R.file_off[(size_t)b0], c1 = R.file_off[(size_t)b1];
  std::vector<BgzfBlk> w(R.blks.begin() + b0, R.blks.begin() + b1);
  for (BgzfBlk& k : w) {
    k.src -= c0;
    k.dst -= dst0;
  }
  R.m_w = w.back().dst + w.back().isize;
  R.b0 = b0;
  R.b1 = b1;
  bqsr_status st;
  if ((st = sam_alloc(R.win, &R.d_raw, (size_t)R.m_w + 64)) != BQSR_OK) return st;
  HIP_TRY(hipMemsetAsync(R.d_raw + R.m_w, 0, 64, s));
  std::vector<int32_t> hs;
  if ((st = bgzf_inflate_runs(R.ctx, R.data + c0, c1 - c0, w, R.d_raw, s, R.win, d_blk, hs)) != BQSR_OK) return st;
  const Deflate& D = Deflate::get();
  std::vector<uint8_t> one;
  for (size_t i = 0; i < w.size(); ++i) {
    if (hs[i] == bgzfk::kInfOk || w[i].isize == 0) continue;
    void* dec = D.ok() ? D.alloc() : nullptr;
    one.resize((size_t)w[i].isize);
    const uint8_t* src = R.data + c0 + w[i].src;
    const bool good = (!D.ok() || dec) && inflate_block(D, dec, src, w[i].csize, one.data(), w[i].isize, le32(src + w[i].csize));
    if (dec) D.free(dec);
    if (!good)
      return fail(BQSR_ERR_SAM_PARSE, "BAM: the BGZF block at byte " + std::to_string(R.file_off[(size_t)b0 + i]) +
                                          " does not inflate or fails its CRC32 (read " + std::to_string(R.st.records_seen) +
                                          " or a later one)", R.st.records_seen);
    HIP_TRY(hipMemcpy(R.d_raw + w[i].dst, one.data(), one.size(), hipMemcpyHostToDevice));
    R.st.members_host += 1;
  }
  R.st.members_read += b1 - b0;
  R.have_window = true;
  return BQSR_OK;
}

// the window's complete records from R.start: the device chain, or where its check declines the host's walk
bqsr_status window_chain(bqsr_bam_reader& R, const bgzfk::Blk* d_blk, hipStream_t s, bool& device) {
  const int64_t nb = R.b1 - R.b0;
  bqsr_status st;
  bamw::WindowChain W{};
  bgzfk::ChainParams& C = W.C;
  C.u = R.d_raw;
  C.m = R.m_w;
  C.body = R.start;
  C.blks = d_blk;
  C.n_blk = nb;
  C.n_ref = (int32_t)((int64_t)R.BH.ref_off.size() - 1);
  uint64_t *part, *base;
  if ((st = sam_alloc(R.win, &C.guess, (size_t)nb)) != BQSR_OK || (st = sam_alloc(R.win, &C.exit, (size_t)nb)) != BQSR_OK ||
      (st = sam_alloc(R.win, &C.count, (size_t)nb)) != BQSR_OK || (st = sam_alloc(R.win, &base, (size_t)nb + 1)) != BQSR_OK ||
      (st = sam_alloc(R.win, &part, (size_t)(nb / samk::kScanChunk + 2))) != BQSR_OK ||
      (st = sam_alloc(R.win, &C.bad, 1)) != BQSR_OK || (st = sam_alloc(R.win, &W.stop, 1)) != BQSR_OK)
    return st;
  HIP_TRY(hipMemsetAsync(C.bad, 0, 4, s));
  HIP_TRY(hipMemcpyAsync(W.stop, &R.m_w, 8, hipMemcpyHostToDevice, s));
  const unsigned gb = (unsigned)((nb + 63) / 64);
  JOB_TRY(launch(bamw::bam_window_guess, gb, 64, s, W));
  JOB_TRY(launch(bamw::bam_window_check, gb, 64, s, W));
  if ((st = sam_scan(C.count, nb, base, part, s)) != BQSR_OK) return st;
  int32_t bad = 0;
  uint64_t total = 0;
  int64_t stop = 0;
  HIP_TRY(hipMemcpyAsync(&bad, C.bad, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&total, base + nb, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&stop, W.stop, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (R.start >= R.m_w) {  // nothing after the start: no block holds it, no walk ran
    bad = 0;
    total = 0;
    stop = R.start;
  }
  device = !bad;
  if (device) {
    R.nr = (int64_t)total;
    R.stop = stop;
    if ((st = sam_alloc(R.win, &R.d_rec, (size_t)R.nr + 1)) != BQSR_OK) return st;
    C.base = base;
    C.rec = R.d_rec;
    JOB_TRY(launch(bamw::bam_window_write, gb, 64, s, W));
    const uint64_t end = (uint64_t)(R.stop - R.start);
    HIP_TRY(hipMemcpyAsync(R.d_rec + R.nr, &end, 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BQSR_OK;
  }
  // the host's walk over the window's bytes
  std::vector<uint8_t> raw((size_t)(R.m_w - R.start));
  HIP_TRY(hipMemcpy(raw.data(), R.d_raw + R.start, raw.size(), hipMemcpyDeviceToHost));
  std::vector<uint64_t> rec;
  const int64_t len = (int64_t)raw.size();
  int64_t q = 0;
  while (q + 4 <= len) {
    const int64_t bs = (int32_t)le32(raw.data() + q);
    if (bs < 32) {
      const int64_t read = R.st.records_seen + (int64_t)rec.size();
      return fail(BQSR_ERR_SAM_PARSE, "BAM: read " + std::to_string(read) + ": bad record size at byte " +
                                          std::to_string(R.blks[(size_t)R.b0].dst + R.start + q) + " of the stream", read);
    }
    if (q + 4 + bs > len) break;
    rec.push_back((uint64_t)q);
    q += 4 + bs;
  }
  R.nr = (int64_t)rec.size();
  R.stop = R.start + q;
  rec.push_back((uint64_t)q);
  if ((st = sam_upload(R.win, &R.d_rec, rec, s)) != BQSR_OK) return st;
  HIP_TRY(hipStreamSynchronize(s));
  return BQSR_OK;
}

// the member that holds stream position p: the last one that starts at or before it
int64_t member_of(const bqsr_bam_reader& R, int64_t p) {
  int64_t a = 0, b = (int64_t)R.blks.size() - 1;
  while (a < b) {
    const int64_t mid = (a + b + 1) >> 1;
    if (R.blks[(size_t)mid].dst <= p) a = mid;
    else b = mid - 1;
  }
  return a;
}

// *p grown to `want` elements (and `pad` bytes), the `used` it holds copied over
template <class T>
bqsr_status keep_grow(T** p, int64_t& cap, int64_t used, int64_t want, size_t pad, hipStream_t s) {
  if (cap >= want) return BQSR_OK;
  const int64_t c = std::max<int64_t>(want, 2 * cap);
  T* q = nullptr;
  if (hipMalloc((void**)&q, (size_t)c * sizeof(T) + pad) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BQSR_ERR_UNSUPPORTED, "BAM region: the region's records stay resident on the device and do not fit: " +
                                          std::to_string((size_t)c * sizeof(T)) + " bytes");
  }
  hipError_t e = hipSuccess;
  if (used > 0) e = hipMemcpyAsync(q, *p, (size_t)used * sizeof(T), hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipFree(q);
    return fail(BQSR_ERR_DEVICE, std::string("BAM region: ") + hipGetErrorString(e));
  }
  if (*p) (void)hipFree(*p);
  *p = q;
  cap = c;
  return BQSR_OK;
}
// room for `bytes` more kept bytes and `n` more kept records (and the terminal offset)
bqsr_status keep_reserve(bqsr_bam_reader& R, int64_t bytes, int64_t n, hipStream_t s) {
  JOB_TRY(keep_grow(&R.keep, R.keep_cap, R.keep_bytes, R.keep_bytes + bytes + 1, 64, s));
  JOB_TRY(keep_grow(&R.keep_rec, R.keep_rec_cap, R.keep_n, R.keep_n + n + 1, 0, s));
  return BQSR_OK;
}

}  // namespace

extern "C" {

bqsr_status bqsr_bam_reader_open(bqsr_context* ctx, const uint8_t* bam, int64_t n_bytes, int64_t piece_bytes,
                                 void* stream, bqsr_bam_reader** out) {
  if (!ctx || !out || n_bytes < 0 || (n_bytes > 0 && !bam) || piece_bytes < 1 || piece_bytes > (int64_t(1) << 31))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_reader_open: bad arguments (piece_bytes is 1 .. 2^31)");
  *out = nullptr;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  std::unique_ptr<bqsr_bam_reader> Rp(new (std::nothrow) bqsr_bam_reader);
  if (!Rp) return fail(BQSR_ERR_DEVICE, "bqsr_bam_reader_open: out of host memory");
  bqsr_bam_reader& R = *Rp;
  R.ctx = ctx;
  R.data = bam;
  R.n = n_bytes;
  R.piece = piece_bytes;
  JOB_TRY(bgzf_blocks(bam, n_bytes, R.blks, R.m));
  if (R.m < 12) return fail(BQSR_ERR_SAM_PARSE, "BAM: no BAM magic");
  const int64_t nb = (int64_t)R.blks.size();
  R.file_off.resize((size_t)nb + 1);
  for (int64_t i = 0; i < nb; ++i) {  // (a member's header is what lies between the one before it and its data)
    const int64_t prev_end = i ? R.blks[(size_t)i - 1].src + R.blks[(size_t)i - 1].csize + 8 : 0;
    R.file_off[(size_t)i] = prev_end;
  }
  R.file_off[(size_t)nb] = n_bytes;
  R.st.members_total = nb;
  R.st.stream_bytes = R.m;
  // the header, from windows of the file's first members until it parses
  std::vector<uint8_t> head;
  for (int64_t want = 1 << 16;; want *= 4) {
    int64_t b1 = 1;
    while (b1 < nb && R.blks[(size_t)b1].dst < want) ++b1;
    bgzfk::Blk* d_blk;
    JOB_TRY(window_inflate(R, 0, b1, s, &d_blk));
    head.resize((size_t)R.m_w);
    HIP_TRY(hipMemcpy(head.data(), R.d_raw, head.size(), hipMemcpyDeviceToHost));
    bqsr_status e;
    const int r = bam_head(head.data(), R.m_w, b1 == nb, R.BH, e);
    if (r < 0) return e;
    if (r == 1) break;
  }
  R.st.members_read = 0;  // (the header's windows are not a read of records)
  int64_t lt = R.BH.l_text;
  while (lt > 0 && head[(size_t)(8 + lt - 1)] == 0) --lt;
  JOB_TRY(parse_sam_header((const char*)head.data() + 8, lt, &R.H));
  R.hdr.assign((const char*)head.data() + 8, (size_t)lt);
  R.drop_window();
  R.p = R.BH.body;
  R.st.n_ref = (int64_t)R.BH.ref_off.size() - 1;
  R.st.body = R.BH.body;
  *out = Rp.release();
  return ok();
}

void bqsr_bam_reader_destroy(bqsr_bam_reader* r) {
  if (!r) return;
  (void)hipSetDevice(r->ctx->device);
  delete r;
}

bqsr_status bqsr_bam_reader_members(const bqsr_bam_reader* r, uint64_t* members, int64_t cap) {
  if (!r || !members) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_reader_members: bad arguments");
  const int64_t nb = (int64_t)r->blks.size();
  if (cap < 2 * (nb + 1)) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_reader_members: the table does not fit");
  for (int64_t i = 0; i < nb; ++i) {
    members[2 * i] = (uint64_t)r->blks[(size_t)i].dst;
    members[2 * i + 1] = (uint64_t)r->file_off[(size_t)i];
  }
  members[2 * nb] = (uint64_t)r->m;
  members[2 * nb + 1] = (uint64_t)r->n;
  return ok();
}

bqsr_status bqsr_bam_reader_seek(bqsr_bam_reader* r, int64_t member, int64_t offset) {
  if (!r || member < 0 || member >= (int64_t)r->blks.size() || offset < 0 ||
      offset > r->blks[(size_t)member].isize)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_reader_seek: no such position in the file's members");
  r->p = r->blks[(size_t)member].dst + offset;
  return ok();
}

bqsr_status bqsr_bam_reader_next(bqsr_bam_reader* r, int64_t end_member, void* stream, bqsr_bam_window* out) {
  if (!r || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_reader_next: bad arguments");
  bqsr_bam_reader& R = *r;
  HIP_TRY(hipSetDevice(R.ctx->device));
  hipStream_t s = S(stream);
  const int64_t nb = (int64_t)R.blks.size();
  *out = bqsr_bam_window{0, 0, 0, R.p, 0, 1};
  R.drop_window();
  if (R.p >= R.m) return ok();
  const int64_t b0 = member_of(R, R.p);
  const int64_t lim = std::min(nb, std::max(end_member, b0 + 1));
  int64_t b1 = b0 + 1;
  while (b1 < lim && R.blks[(size_t)b1].dst + R.blks[(size_t)b1].isize - R.blks[(size_t)b0].dst <= R.piece) ++b1;
  bool device = false;
  for (;;) {
    bgzfk::Blk* d_blk;
    JOB_TRY(window_inflate(R, b0, b1, s, &d_blk));
    R.start = R.p - R.blks[(size_t)b0].dst;
    JOB_TRY(window_chain(R, d_blk, s, device));
    if (R.nr > 0) break;
    // no whole record yet: the window grows, member by member, to what the first record's size word asks for
    if (b1 == nb)
      return fail(BQSR_ERR_SAM_PARSE, "BAM: truncated record: read " + std::to_string(R.st.records_seen) +
                                          " does not end inside the file", R.st.records_seen);
    int64_t need = R.m_w + 1;
    if (R.start + 4 <= R.m_w) {
      uint8_t w4[4];
      HIP_TRY(hipMemcpy(w4, R.d_raw + R.start, 4, hipMemcpyDeviceToHost));
      const int64_t bs = (int32_t)le32(w4);
      if (R.p + 4 + bs > R.m)  // (what the size word asks for is not in the file: nothing more is inflated for it)
        return fail(BQSR_ERR_SAM_PARSE, "BAM: truncated record: read " + std::to_string(R.st.records_seen) +
                                            " does not end inside the file", R.st.records_seen);
      need = std::max<int64_t>(need, R.start + 4 + bs);
    }
    R.st.members_read -= b1 - b0;  // (the window is inflated again, larger: its members count once)
    ++b1;
    while (b1 < nb && R.blks[(size_t)b1 - 1].dst + R.blks[(size_t)b1 - 1].isize - R.blks[(size_t)b0].dst < need) ++b1;
  }
  (device ? R.st.windows_device : R.st.windows_host) += 1;
  R.first = R.st.records_seen;
  R.st.records_seen += R.nr;
  R.p = R.blks[(size_t)b0].dst + R.stop;
  *out = bqsr_bam_window{R.nr, b0, b1, R.p, device ? 1 : 0, R.p >= R.m ? 1 : 0};
  return ok();
}

bqsr_status bqsr_bam_index_add_window(bqsr_bam_index* x, bqsr_bam_reader* r, void* stream) {
  if (!x || !r || !r->have_window || !r->d_rec)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_add_window before bqsr_bam_reader_next");
  bqsr_bam_index& X = *x;
  bqsr_bam_reader& R = *r;
  if (X.has_members || X.finished) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_add_window after the member table");
  const uint64_t base = (uint64_t)(R.blks[(size_t)R.b0].dst + R.start);
  if (base < X.stream_end && X.n_rows > 0)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_index_add_window: a window that starts before the end of the one before it");
  if (X.n_rows + R.nr > (int64_t)0xFFFFFFFFll)
    return fail(BQSR_ERR_UNSUPPORTED, "BAM index: more than 2^32 - 1 records in one index");
  HIP_TRY(hipSetDevice(X.ctx->device));
  X.on_device = true;
  hipStream_t st = S(stream);
  bai_rows_time(X);
  JOB_TRY(bai_rows_reserve(X, R.nr, st));
  if (R.nr > 0) {
    unsigned long long* err;
    JOB_TRY(dev_need(X.err, &err, 1, "BAM index", "status word"));
    HIP_TRY(hipMemsetAsync(err, 0xFF, 8, st));
    baik::RawRowsParams A{R.d_raw + R.start, R.d_rec, R.nr, X.rows + X.n_rows, base, R.first, err};
    HIP_TRY(X.clock.mark(BAI_ROWS_0, st));
    JOB_TRY(launch(baik::bai_rows_raw, sam_grid(R.nr, baik::kThreads, X.ctx->n_cu * 8), baik::kThreads, st, A));
    HIP_TRY(X.clock.mark(BAI_ROWS_1, st));
    X.rows_timed = false;
    unsigned long long ew = ~0ull;
    HIP_TRY(hipMemcpyAsync(&ew, err, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the window's buffers are released at the next one)
    if (ew != ~0ull)
      return fail(BQSR_ERR_SAM_PARSE, "BAM: read " + std::to_string((long long)(ew >> 8)) +
                                          ": its name and CIGAR do not fit its block_size", (int64_t)(ew >> 8));
  }
  X.n_rows += R.nr;
  X.stream_end = (uint64_t)(R.blks[(size_t)R.b0].dst + R.stop);
  return ok();
}

bqsr_status bqsr_bam_reader_filter(bqsr_bam_reader* r, int32_t ref, int64_t beg, int64_t end, int64_t limit,
                                   void* stream, int64_t* kept, int32_t* done) {
  if (!r || !kept || !done || !r->have_window || !r->d_rec || ref < 0 || beg < 0 || end <= beg || end > (int64_t(1) << 29))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_reader_filter: bad arguments, or before bqsr_bam_reader_next");
  bqsr_bam_reader& R = *r;
  HIP_TRY(hipSetDevice(R.ctx->device));
  hipStream_t s = S(stream);
  *kept = 0;
  *done = 0;
  if (R.nr == 0) return ok();
  bqsr_status st;
  bamw::FilterParams F{};
  F.buf = R.d_raw + R.start;
  F.rec = R.d_rec;
  F.n = R.nr;
  F.base = (uint64_t)(R.blks[(size_t)R.b0].dst + R.start);
  F.limit = (uint64_t)limit;
  F.rid = ref;
  F.rbeg = (uint32_t)beg;
  F.rend = (uint32_t)end;
  F.first = R.first;
  uint64_t *off, *part;
  unsigned long long* words;  // stop, err
  if ((st = sam_alloc(R.win, &F.len, (size_t)R.nr)) != BQSR_OK || (st = sam_alloc(R.win, &off, (size_t)R.nr + 1)) != BQSR_OK ||
      (st = sam_alloc(R.win, &part, (size_t)(R.nr / samk::kScanChunk + 2))) != BQSR_OK ||
      (st = sam_alloc(R.win, &words, 2)) != BQSR_OK)
    return st;
  F.stop = words;
  F.err = words + 1;
  HIP_TRY(hipMemsetAsync(words, 0xFF, 16, s));
  const unsigned g = sam_grid(R.nr, bamw::kThreads, R.ctx->n_cu * 8);
  HIP_TRY(R.clock.mark(0, s));
  JOB_TRY(launch(bamw::region_filter, g, bamw::kThreads, s, F));
  unsigned long long hw[2] = {~0ull, ~0ull};
  HIP_TRY(hipMemcpyAsync(hw, words, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (hw[1] != ~0ull)
    return fail(BQSR_ERR_SAM_PARSE, "BAM: read " + std::to_string((long long)(hw[1] >> 8)) +
                                        " of the reads seen: its name and CIGAR do not fit its block_size", (int64_t)(hw[1] >> 8));
  int64_t n_eff = R.nr;
  if (hw[0] != ~0ull) {
    n_eff = (int64_t)(hw[0] >> 1);
    *done = (hw[0] & 1ull) ? 1 : 2;  // 1: the chunk is over; 2: the region is
  }
  if (n_eff == 0) return ok();
  if ((st = sam_scan(F.len, n_eff, off, part, s)) != BQSR_OK) return st;
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, off + n_eff, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int64_t nk = (int64_t)(total >> bamw::kCountShift), nbytes = (int64_t)(total & bamw::kBytesMask);
  if (nk > 0) {
    JOB_TRY(keep_reserve(R, nbytes, nk, s));
    bamw::CopyParams C{F.buf, F.rec, F.len, off, n_eff, R.keep + R.keep_bytes, R.keep_rec + R.keep_n, (uint64_t)R.keep_bytes};
    JOB_TRY(launch(bamw::region_copy, sam_grid(n_eff, bamw::kThreads, R.ctx->n_cu * 8), bamw::kThreads, s, C));
    HIP_TRY(R.clock.mark(1, s));
    HIP_TRY(hipStreamSynchronize(s));
    R.clock.add(R.st.filter_ms, 0, 1);
    R.keep_bytes += nbytes;
    R.keep_n += nk;
    R.st.records_kept += nk;
  }
  *kept = nk;
  return ok();
}

bqsr_status bqsr_bam_reader_parse(bqsr_bam_reader* r, void* stream, bqsr_sam** out) {
  if (!r || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_reader_parse: bad arguments");
  bqsr_bam_reader& R = *r;
  HIP_TRY(hipSetDevice(R.ctx->device));
  hipStream_t s = S(stream);
  R.drop_window();
  JOB_TRY(keep_reserve(R, 0, 0, s));
  const uint64_t end = (uint64_t)R.keep_bytes;
  HIP_TRY(hipMemcpyAsync(R.keep_rec + R.keep_n, &end, 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(R.keep + R.keep_bytes, 0, 64, s));
  std::vector<void*> tmp;
  struct Free {
    std::vector<void*>& v;
    ~Free() {
      for (void* q : v) (void)hipFree(q);
    }
  } free_tmp{tmp};
  uint8_t* d_text = nullptr;
  int64_t n_text = 0;
  std::string hdr = R.hdr;
  SamHeader H = R.H;
  JOB_TRY(bam_lines_text(R.ctx, R.keep, R.keep_rec, R.keep_n, R.BH, H, hdr, s, tmp, &d_text, &n_text));
  const bqsr_status st = sam_parse_device(R.ctx, H, hdr.data(), d_text, n_text, s, true, out);  // (owns d_text from here)
  if (st == BQSR_OK) (*out)->bam_form = R.st.members_host > 0 ? 1 : 2;  // (1: a member came from the host's inflate)
  return st;
}

bqsr_status bqsr_bam_reader_get_stats(const bqsr_bam_reader* r, bqsr_bam_reader_stats* out) {
  if (!r || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bam_reader_get_stats: bad arguments");
  *out = r->st;
  return ok();
}

}  // extern "C"
