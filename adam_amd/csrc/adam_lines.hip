// ADAMRecord Parquet -> SAM text on the device (include/adam_sam.h
// bqsr_arrow_sam_lines): the inverse of SAMRecordConverter.convert
// (core/converters/SAMRecordConverter.scala:26-144), so that ADAM input
// reaches the SAM and BAM sinks the way BAM input does -- every record
// rendered as its SAM line here, the text handed to sam_parse_device
// (bam_ingest.hip does the same for BAM records).  The line's rules, and the
// choices where the converter loses information, are stated in the header.
// Included by bqsr_capi.cpp after arrow_ingest.hip.
//
//   upload : per Arrow record batch, its buffers copied to the device as
//            they are (bit offsets zero: the host flattens sliced arrays);
//   len    : a lane per record: the line's length, and every refusal (the
//            first failing record by atomicMin, as bam_lines_len);
//   scan   : sam_scan over the lengths;
//   write  : a lane per record writes its short fields (the numbers, "*",
//            "=", the reference names, the tabs); the string fields of a
//            wavefront's 64 records are then copied by the whole wavefront,
//            one record after another: offset, destination and length
//            broadcast from the owning lane, the lanes striding over the
//            bytes, so that the stores of a copy are contiguous.  The
//            attribute fields, written in reverse, are found by their owning
//            lanes (all at once, a field from the back a round) and copied
//            the same way.  The loops that broadcast run over whole
//            wavefronts: a lane without a record stays in them with nothing
//            to copy, so no broadcast reads a lane that has left.

namespace adlk {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kBools = 11;
// the string columns, in the order of bqsr_adam_lines_chunk
enum { kName = 0, kCigar = 1, kSeq = 2, kQual = 3, kAttr = 4, kMd = 5, kStrs = 6 };
// the boolean columns, in the order of bqsr_adam_lines_chunk (adam_save.BOOL_COLS)
enum { kPaired = 0, kProper, kMapped, kMateMapped, kNeg, kMateNeg, kFirst, kSecond, kPrimary, kFailedQc, kDup };
enum : uint32_t { kOk = 0, kMalformed = 1, kUnrepresentable = 2 };
constexpr int64_t kMaxStart = 2147483646;  // 2^31 - 2: POS = start + 1 stays an Int

struct Str {
  const int32_t* off;    // [n + 1], as Arrow's (the first need not be 0); null: the column is all null
  const uint8_t* data;   // the bytes of [off[0], off[n])
  const uint8_t* valid;  // null: all valid
  int32_t base;          // off[0]
};

// one record batch's buffers on the device
struct Chunk {
  int64_t n, r0;  // records; the first one's index in the table
  Str s[kStrs];
  const int64_t* start;
  const uint8_t* start_valid;
  const int64_t* mate_start;
  const uint8_t* mate_start_valid;
  const int32_t* mapq;
  const uint8_t* mapq_valid;
  const int32_t* ref;  // indices into the reference names; null or invalid: no name
  const uint8_t* ref_valid;
  const int32_t* mate_ref;
  const uint8_t* mate_ref_valid;
  const uint8_t* bools[kBools];  // value bitmaps or null (false)
  const uint8_t* bools_valid[kBools];
};

struct Params {
  Chunk C;
  const uint8_t* ref_blob;  // reference name i: ref_blob[ref_off[i], ref_off[i + 1])
  const uint64_t* ref_off;
  int32_t n_ref;
  uint64_t* len;            // [table's n] line bytes of record g, '\n' included (pass 1)
  const uint64_t* off;      // [n + 1] their exclusive scan (pass 2)
  uint8_t* out;             // the SAM text: the header at [0, hdr), record g's line at hdr + off[g]
  int64_t hdr;
  unsigned long long* err;  // (record << 8) | code, the smallest wins
};

__device__ __forceinline__ bool bit(const uint8_t* bm, int64_t i) { return !bm || ((bm[i >> 3] >> (i & 7)) & 1u); }
// a record's code: the smallest of what its checks found
__device__ __forceinline__ uint32_t worse(uint32_t bad, uint32_t e) { return e && (!bad || e < bad) ? e : bad; }

// string k of record r: its first byte's offset and its length (0: null or empty)
__device__ __forceinline__ int32_t str_of(const Str& s, int64_t r, int32_t* a) {
  if (!s.off || !bit(s.valid, r)) return 0;
  *a = s.off[r];
  return s.off[r + 1] - *a;
}

// the record's fields that are not strings
struct Rec {
  uint32_t flag;
  int32_t ref, mref;  // -1: none
  int64_t pos, pnext;
  int32_t mapq;
  uint32_t bad;
};

__device__ Rec rec_of(const Params& P, int64_t r) {
  const Chunk& C = P.C;
  Rec R{};
  uint32_t b = 0;
  for (int k = 0; k < kBools; ++k)  // a null boolean reads as false
    if (C.bools[k] && bit(C.bools_valid[k], r) && bit(C.bools[k], r)) b |= 1u << k;
  const auto on = [&](int k) { return (b >> k) & 1u; };
  if (b)  // (all false: FLAG 0, as the converter writes a FLAG of 0)
    R.flag = (on(kPaired) ? 0x1u : 0u) | (on(kProper) ? 0x2u : 0u) | (on(kMapped) ? 0u : 0x4u) |
             (on(kPaired) && !on(kMateMapped) ? 0x8u : 0u) | (on(kNeg) ? 0x10u : 0u) | (on(kMateNeg) ? 0x20u : 0u) |
             (on(kFirst) ? 0x40u : 0u) | (on(kSecond) ? 0x80u : 0u) | (on(kPrimary) ? 0u : 0x100u) |
             (on(kFailedQc) ? 0x200u : 0u) | (on(kDup) ? 0x400u : 0u);
  const bool has_ref = C.ref && bit(C.ref_valid, r), has_mref = C.mate_ref && bit(C.mate_ref_valid, r);
  R.ref = has_ref ? C.ref[r] : -1;
  R.mref = has_mref ? C.mate_ref[r] : -1;
  if ((has_ref && (R.ref < 0 || R.ref >= P.n_ref)) || (has_mref && (R.mref < 0 || R.mref >= P.n_ref))) {
    R.bad = kMalformed;
    R.ref = R.mref = -1;  // (no name is read)
  }
  if (C.start && bit(C.start_valid, r)) {
    const int64_t v = C.start[r];
    if (v < 0 || v > kMaxStart) R.bad = worse(R.bad, kUnrepresentable);
    R.pos = v + 1;
  }
  if (C.mate_start && bit(C.mate_start_valid, r)) {
    const int64_t v = C.mate_start[r];
    if (v < 0 || v > kMaxStart) R.bad = worse(R.bad, kUnrepresentable);
    R.pnext = v + 1;
  }
  if (C.mapq && bit(C.mapq_valid, r)) {
    R.mapq = C.mapq[r];
    if (R.mapq < 0 || R.mapq > 255) R.bad = worse(R.bad, kUnrepresentable);
  } else {
    R.mapq = R.ref >= 0 ? 255 : 0;  // (the converter drops a MAPQ of 255, and only on a placed read)
  }
  return R;
}

__device__ __forceinline__ void ref_name(const Params& P, bamk::Put& o, int32_t id) {
  if (id >= 0) o.bytes(P.ref_blob + P.ref_off[id], (int64_t)(P.ref_off[id + 1] - P.ref_off[id]));
  else o.c('*');
}
// "\tFLAG\tRNAME\tPOS\tMAPQ\t" (between QNAME and CIGAR)
__device__ void put_head(const Params& P, bamk::Put& o, const Rec& R) {
  o.c('\t');
  o.integer(R.flag);
  o.c('\t');
  ref_name(P, o, R.ref);
  o.c('\t');
  o.integer(R.pos);
  o.c('\t');
  o.integer(R.mapq);
  o.c('\t');
}
// "\tRNEXT\tPNEXT\tTLEN\t" (between CIGAR and SEQ; ADAMRecord has no TLEN)
__device__ void put_mid(const Params& P, bamk::Put& o, const Rec& R) {
  o.c('\t');
  if (R.mref >= 0 && R.mref == R.ref) o.c('=');
  else ref_name(P, o, R.mref);
  o.c('\t');
  o.integer(R.pnext);
  o.c('\t');
  o.c('0');
  o.c('\t');
}

__device__ __forceinline__ bool is_alpha(uint8_t c) { return (uint8_t)((c | 0x20) - 'a') < 26; }
__device__ __forceinline__ bool is_digit(uint8_t c) { return (uint8_t)(c - '0') < 10; }

// a field's bytes may not hold what ends a SAM field or line
__device__ uint32_t check_field(const uint8_t* p, int32_t n) {
  for (int32_t i = 0; i < n; ++i)
    if (p[i] == '\t' || p[i] == '\n' || p[i] == '\r') return kUnrepresentable;
  return kOk;
}
// attributes: fields cut at TAB, each [A-Za-z][A-Za-z0-9]:[AifZHB]:...
__device__ uint32_t check_attributes(const uint8_t* p, int32_t n) {
  uint32_t bad = kOk;
  for (int32_t a = 0; a <= n;) {
    int32_t b = a;
    while (b < n && p[b] != '\t') {
      if (p[b] == '\n' || p[b] == '\r') bad = kUnrepresentable;
      ++b;
    }
    const uint8_t t = b - a >= 5 ? p[a + 3] : 0;
    if (b - a < 5 || !is_alpha(p[a]) || !(is_alpha(p[a + 1]) || is_digit(p[a + 1])) || p[a + 2] != ':' || p[a + 4] != ':' ||
        !(t == 'A' || t == 'i' || t == 'f' || t == 'Z' || t == 'H' || t == 'B'))
      return kMalformed;
    a = b + 1;
  }
  return bad;
}

extern "C" __global__ void __launch_bounds__(kThreads) adam_lines_len(Params P) {
  const Chunk& C = P.C;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < C.n; r += (int64_t)gridDim.x * blockDim.x) {
    const Rec R = rec_of(P, r);
    uint32_t bad = R.bad;
    bamk::Put o{nullptr, 0};
    put_head(P, o, R);
    put_mid(P, o, R);
    for (int k = 0; k < kStrs; ++k) {
      int32_t a = 0;
      const int32_t n = str_of(C.s[k], r, &a);
      const uint8_t* p = C.s[k].data + (a - C.s[k].base);
      if (k == kAttr) {
        if (n > 0) {
          bad = worse(bad, check_attributes(p, n));
          o.n += (int64_t)n + 1;  // a TAB before every field
        }
      } else {
        bad = worse(bad, check_field(p, n));
        if (k == kMd) o.n += C.s[k].off && bit(C.s[k].valid, r) ? 6 + (int64_t)n : 0;  // "\tMD:Z:" and the value
        else o.n += n > 0 ? (int64_t)n : 1;  // ("*")
      }
    }
    o.n += 2;  // the TAB between SEQ and QUAL, and '\n'
    if (bad) atomicMin(P.err, ((unsigned long long)(C.r0 + r) << 8) | bad);
    P.len[C.r0 + r] = bad ? 0 : (uint64_t)o.n;
  }
}

__device__ __forceinline__ int64_t bcast64(int64_t v, int lane) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane, kWave);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), lane, kWave);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The wavefront copies, one owning lane after another (the set bits of m,
// the same in every lane): n bytes from src + a to out + d, all three the
// owner's.  Every lane of the wavefront is here.
__device__ __forceinline__ void wave_copy(unsigned long long m, const uint8_t* src, int32_t a, int32_t n, uint8_t* out,
                                          int64_t d, int lane) {
  while (m) {
    const int j = __ffsll((long long)m) - 1;
    m &= m - 1;
    const int32_t ja = __shfl(a, j, kWave), jn = __shfl(n, j, kWave);
    const int64_t jd = bcast64(d, j);
    const uint8_t* q = src + ja;
    for (int32_t i = lane; i < jn; i += kWave) out[jd + i] = q[i];
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) adam_lines_write(Params P) {
  const Chunk& C = P.C;
  const int lane = threadIdx.x & (kWave - 1);
  // whole wavefronts: 64 consecutive records a step, the bounds the same in every lane
  for (int64_t w0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x - lane); w0 < C.n; w0 += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = w0 + lane;
    const bool live = r < C.n;
    int32_t sa[kStrs] = {0, 0, 0, 0, 0, 0}, sn[kStrs] = {0, 0, 0, 0, 0, 0};  // what the wavefront copies: offset, length
    int64_t sd[kStrs] = {0, 0, 0, 0, 0, 0};                                  // and where to (an index into P.out)
    int32_t attr_a = 0, attr_n = 0;  // the attributes: their offset, the bytes not yet written
    int64_t attr_d = 0;              // where the next attribute field's TAB goes
    if (live) {
      const Rec R = rec_of(P, r);
      const int64_t line = P.hdr + (int64_t)P.off[C.r0 + r];
      bamk::Put o{P.out + line, 0};
      const auto str = [&](int k) {  // "*" by the lane, anything longer left to the wavefront
        int32_t a = 0;
        const int32_t n = str_of(C.s[k], r, &a);
        if (n > 0) {
          sa[k] = a - C.s[k].base;
          sn[k] = n;
          sd[k] = line + o.n;
          o.n += n;
        } else {
          o.c('*');
        }
      };
      str(kName);
      put_head(P, o, R);
      str(kCigar);
      put_mid(P, o, R);
      str(kSeq);
      o.c('\t');
      str(kQual);
      attr_n = str_of(C.s[kAttr], r, &attr_a);
      attr_a -= C.s[kAttr].base;
      attr_d = line + o.n;
      if (attr_n > 0) o.n += (int64_t)attr_n + 1;
      if (C.s[kMd].off && bit(C.s[kMd].valid, r)) {
        const uint8_t tag[6] = {'\t', 'M', 'D', ':', 'Z', ':'};
        o.bytes(tag, 6);
        int32_t a = 0;
        const int32_t n = str_of(C.s[kMd], r, &a);
        sa[kMd] = a - C.s[kMd].base;
        sn[kMd] = n;
        sd[kMd] = line + o.n;
        o.n += n;
      }
      o.c('\n');
    }
#pragma unroll
    for (int k = 0; k < kStrs; ++k)
      if (k != kAttr) wave_copy(__ballot(sn[k] > 0), C.s[k].data, sa[k], sn[k], P.out, sd[k], lane);
    // the attribute fields from the back, a field of every record a round
    for (;;) {
      const unsigned long long m = __ballot(attr_n > 0);
      if (!m) break;
      int32_t fa = 0, fn = 0;
      int64_t fd = 0;
      if (attr_n > 0) {
        const uint8_t* p = C.s[kAttr].data + attr_a;
        int32_t a = attr_n;
        while (a > 0 && p[a - 1] != '\t') --a;
        P.out[attr_d] = '\t';
        fa = attr_a + a;
        fn = attr_n - a;
        fd = attr_d + 1;
        attr_d += 1 + (int64_t)fn;
        attr_n = a > 0 ? a - 1 : 0;
      }
      wave_copy(m, C.s[kAttr].data, fa, fn, P.out, fd, lane);
    }
  }
}

}  // namespace adlk

namespace {

enum { ADL_UPLOAD = 0, ADL_LEN, ADL_WRITE, ADL_PARSE, ADL_STAGES };
enum { ADL_T0 = 0, ADL_T_UP, ADL_T_LEN, ADL_T_W0, ADL_T_W1, ADL_MARKS };
thread_local double g_adam_lines_ms[ADL_STAGES] = {0.0, 0.0, 0.0, 0.0};

// an Arrow buffer of `count` elements to the device (null stays null)
template <class T>
bqsr_status adl_h2d(std::vector<void*>& keep, const T** dst, const T* src, size_t count, hipStream_t s) {
  *dst = nullptr;
  if (!src) return BQSR_OK;
  T* d;
  JOB_TRY(sam_alloc(keep, &d, count));
  if (count) HIP_TRY(hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, s));
  *dst = d;
  return BQSR_OK;
}

}  // namespace

bqsr_status bqsr_arrow_sam_lines(bqsr_context* ctx, const bqsr_adam_lines_chunk* chunks, int32_t n_chunks,
                                 const uint8_t* ref_names_blob, const int64_t* ref_name_offsets, int32_t n_ref,
                                 const char* header, int64_t header_bytes, void* stream, bqsr_sam** out) {
  using namespace adlk;
  if (!ctx || !out || n_chunks < 0 || (n_chunks && !chunks) || n_ref < 0 || (n_ref && !ref_name_offsets) ||
      header_bytes < 0 || (header_bytes && !header))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_sam_lines: bad arguments");
  *out = nullptr;
  for (int32_t i = 0; i < n_ref; ++i)
    if (ref_name_offsets[i] < 0 || ref_name_offsets[i + 1] < ref_name_offsets[i] ||
        (ref_name_offsets[i + 1] > 0 && !ref_names_blob))
      return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_sam_lines: bad reference name offsets");
  int64_t n = 0;
  for (int32_t c = 0; c < n_chunks; ++c) {
    const bqsr_adam_lines_chunk& H = chunks[c];
    if (H.n_reads < 0) return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_sam_lines: negative chunk length");
    const bqsr_arrow_strings* sc[kStrs] = {&H.read_name, &H.cigar, &H.sequence, &H.qual, &H.attributes, &H.md};
    for (int k = 0; k < kStrs; ++k)
      if (sc[k]->offsets) {
        const int32_t a = sc[k]->offsets[0], b = sc[k]->offsets[H.n_reads];
        if (a < 0 || b < a || (b > a && !sc[k]->data))
          return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_sam_lines: bad string offsets");
      }
    n += H.n_reads;
  }
  // the header: header lines only, newline-terminated
  std::string hdr(header ? header : "", (size_t)header_bytes);
  if (!hdr.empty() && hdr.back() != '\n') hdr.push_back('\n');
  SamHeader H;
  JOB_TRY(parse_sam_header(hdr.data(), (int64_t)hdr.size(), &H));
  if (H.body != (int64_t)hdr.size())
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_sam_lines: the header holds a line that is not a header line");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  for (double& v : g_adam_lines_ms) v = 0.0;
  StageClock<ADL_MARKS> clock;
  std::vector<void*> tmp;
  struct Free {
    std::vector<void*>& v;
    ~Free() {
      for (void* q : v) (void)hipFree(q);
    }
  } free_tmp{tmp};
  HIP_TRY(clock.mark(ADL_T0, s));
  // ---- every record batch's buffers, as they are ----
  Params P{};
  {
    std::vector<uint8_t> blob(ref_names_blob, ref_names_blob + (n_ref ? ref_name_offsets[n_ref] : 0));
    if (blob.empty()) blob.push_back(0);
    std::vector<uint64_t> off((size_t)n_ref + 1, 0);
    for (int32_t i = 0; i <= n_ref && n_ref; ++i) off[(size_t)i] = (uint64_t)ref_name_offsets[i];
    JOB_TRY(sam_upload(tmp, (uint8_t**)&P.ref_blob, blob, s));
    JOB_TRY(sam_upload(tmp, (uint64_t**)&P.ref_off, off, s));
    HIP_TRY(hipStreamSynchronize(s));  // (the copies read `blob` and `off`)
  }
  P.n_ref = n_ref;
  std::vector<Chunk> dev;
  int64_t r0 = 0;
  for (int32_t c = 0; c < n_chunks; ++c) {
    const bqsr_adam_lines_chunk& A = chunks[c];
    const int64_t m = A.n_reads;
    if (m == 0) continue;
    const size_t vb = (size_t)(m + 7) / 8;
    Chunk D{};
    D.n = m;
    D.r0 = r0;
    const bqsr_arrow_strings* sc[kStrs] = {&A.read_name, &A.cigar, &A.sequence, &A.qual, &A.attributes, &A.md};
    for (int k = 0; k < kStrs; ++k) {
      if (!sc[k]->offsets) continue;
      const int32_t a = sc[k]->offsets[0], b = sc[k]->offsets[m];
      D.s[k].base = a;
      JOB_TRY(adl_h2d(tmp, &D.s[k].off, sc[k]->offsets, (size_t)m + 1, s));
      JOB_TRY(adl_h2d(tmp, &D.s[k].valid, sc[k]->validity, vb, s));
      uint8_t* d;
      JOB_TRY(sam_alloc(tmp, &d, (size_t)(b - a)));
      if (b > a) JOB_TRY(upload_staged(ctx, d, sc[k]->data + a, (size_t)(b - a), s));
      D.s[k].data = d;
    }
    JOB_TRY(adl_h2d(tmp, &D.start, A.start, (size_t)m, s));
    JOB_TRY(adl_h2d(tmp, &D.start_valid, A.start ? A.start_validity : nullptr, vb, s));
    JOB_TRY(adl_h2d(tmp, &D.mate_start, A.mate_start, (size_t)m, s));
    JOB_TRY(adl_h2d(tmp, &D.mate_start_valid, A.mate_start ? A.mate_start_validity : nullptr, vb, s));
    JOB_TRY(adl_h2d(tmp, &D.mapq, A.mapq, (size_t)m, s));
    JOB_TRY(adl_h2d(tmp, &D.mapq_valid, A.mapq ? A.mapq_validity : nullptr, vb, s));
    JOB_TRY(adl_h2d(tmp, &D.ref, A.reference, (size_t)m, s));
    JOB_TRY(adl_h2d(tmp, &D.ref_valid, A.reference ? A.reference_validity : nullptr, vb, s));
    JOB_TRY(adl_h2d(tmp, &D.mate_ref, A.mate_reference, (size_t)m, s));
    JOB_TRY(adl_h2d(tmp, &D.mate_ref_valid, A.mate_reference ? A.mate_reference_validity : nullptr, vb, s));
    for (int k = 0; k < kBools; ++k) {
      JOB_TRY(adl_h2d(tmp, &D.bools[k], A.bools[k], vb, s));
      JOB_TRY(adl_h2d(tmp, &D.bools_valid[k], A.bools[k] ? A.bools_validity[k] : nullptr, vb, s));
    }
    dev.push_back(D);
    r0 += m;
  }
  HIP_TRY(clock.mark(ADL_T_UP, s));
  // ---- pass 1: the lines' lengths, and every refusal ----
  uint64_t *len, *off, *part;
  JOB_TRY(sam_alloc(tmp, &len, (size_t)n));
  JOB_TRY(sam_alloc(tmp, &off, (size_t)n + 1));
  JOB_TRY(sam_alloc(tmp, &part, (size_t)(n / samk::kScanChunk + 2)));
  JOB_TRY(sam_alloc(tmp, &P.err, 1));
  HIP_TRY(hipMemsetAsync(P.err, 0xFF, 8, s));
  P.len = len;
  P.off = off;
  P.hdr = (int64_t)hdr.size();
  for (const Chunk& D : dev) {
    P.C = D;
    JOB_TRY(launch(adam_lines_len, sam_grid(D.n, kThreads, ctx->n_cu * 16), kThreads, s, P));
  }
  HIP_TRY(clock.mark(ADL_T_LEN, s));
  JOB_TRY(sam_scan(len, n, off, part, s));
  unsigned long long e_word = ~0ull;
  uint64_t body_bytes = 0;
  HIP_TRY(hipMemcpyAsync(&e_word, P.err, 8, hipMemcpyDeviceToHost, s));
  if (n > 0) HIP_TRY(hipMemcpyAsync(&body_bytes, off + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (e_word != ~0ull) {
    const uint32_t code = (uint32_t)(e_word & 0xFF);
    const int64_t read = (int64_t)(e_word >> 8);
    char buf[200];
    snprintf(buf, sizeof buf, "ADAM record %lld: %s", (long long)read,
             code == kMalformed ? "malformed record (an attribute that is not TG:T:value, or a reference index "
                                  "outside the names)"
                                : "a record SAM cannot hold (TAB, LF or CR inside a field, start or "
                                  "mateAlignmentStart outside [0, 2^31 - 2], or mapq outside [0, 255])");
    return fail(code == kMalformed ? BQSR_ERR_SAM_PARSE : BQSR_ERR_UNSUPPORTED, buf, read);
  }
  // ---- pass 2: the text ----
  const int64_t n_text = P.hdr + (int64_t)body_bytes;
  uint8_t* d_text = nullptr;
  if (hipMalloc(&d_text, (size_t)n_text + 64) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BQSR_ERR_UNSUPPORTED, "bqsr_arrow_sam_lines: one input stays resident on the device and this one does "
                                      "not fit: " + std::to_string(n_text) + " bytes for its SAM text");
  }
  hipError_t e = hipMemsetAsync(d_text + n_text, 0, 64, s);
  if (e == hipSuccess && P.hdr > 0) e = hipMemcpyAsync(d_text, hdr.data(), hdr.size(), hipMemcpyHostToDevice, s);
  P.out = d_text;
  if (e == hipSuccess) e = clock.mark(ADL_T_W0, s);
  for (const Chunk& D : dev) {
    if (e != hipSuccess) break;
    P.C = D;
    e = launch_err(adam_lines_write, sam_grid(D.n, kThreads, ctx->n_cu * 16), kThreads, s, P);
  }
  if (e == hipSuccess) e = clock.mark(ADL_T_W1, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // (the header copy reads `hdr`)
  if (e != hipSuccess) {
    (void)hipFree(d_text);
    return fail(BQSR_ERR_DEVICE, std::string("bqsr_arrow_sam_lines: ") + hipGetErrorString(e));
  }
  clock.add(g_adam_lines_ms[ADL_UPLOAD], ADL_T0, ADL_T_UP);
  clock.add(g_adam_lines_ms[ADL_LEN], ADL_T_UP, ADL_T_LEN);
  clock.add(g_adam_lines_ms[ADL_WRITE], ADL_T_W0, ADL_T_W1);
  for (void* q : tmp) (void)hipFree(q);  // (the parse allocates its columns next)
  tmp.clear();
  const double t_parse = now_s();
  const bqsr_status st = sam_parse_device(ctx, H, hdr.data(), d_text, n_text, s, false, out);  // (owns d_text from here)
  g_adam_lines_ms[ADL_PARSE] = (now_s() - t_parse) * 1e3;
  return st;
}

bqsr_status bqsr_adam_lines_kernel_times(double* upload_ms, double* len_ms, double* write_ms, double* parse_ms) {
  if (upload_ms) *upload_ms = g_adam_lines_ms[ADL_UPLOAD];
  if (len_ms) *len_ms = g_adam_lines_ms[ADL_LEN];
  if (write_ms) *write_ms = g_adam_lines_ms[ADL_WRITE];
  if (parse_ms) *parse_ms = g_adam_lines_ms[ADL_PARSE];
  return ok();
}
