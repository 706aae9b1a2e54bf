// BAM records from a parse's SAM lines (SAM spec §4.2): the sink that turns
// `transform`'s result back into the format its consumers read.
//
// After bqsr_sam_rewrite_quals / bqsr_sam_sort the parse's device text holds
// every record's final line (a BAM-born parse holds SAM lines too), so a BAM
// record is a function of the line, the parse's CIGAR words and its @SQ index.
// Two passes as adam_out.hip: pass 1 validates a record and computes its
// block_size + 4, a u64 exclusive scan places the records, pass 2 emits the
// bytes.  In pass 2 a lane writes its record's fixed fields, name, CIGAR and
// tags (a serial walk), then the wavefront goes through its 64 records
// together: lane j packs SEQ byte j, j + 64, .. and writes QUAL byte j,
// j + 64, .., so the bulk of the stream leaves in contiguous stores.
//
// Float tags: the stored binary32 must be what C strtof gives for the text.
// The kernel leaves the 4-byte slot, copies the text (NUL-terminated) into a
// side blob and appends (stream offset, blob offset) to a patch list; the
// library converts on the host and fills the slots before the bytes are
// handed out (bqsr_sam_bam_records).
//
// bqsr_bgzf_compress cuts a stream into BGZF members on host threads: the
// seam where a device DEFLATE would go.
//
// Included by bqsr_capi.cpp after adam_out.hip.

namespace bamo {

// error word: (read << 8) | code, the smallest wins
enum : uint32_t {
  kBamOk = 0,
  kBamRname = 1,     // RNAME neither "*" nor an @SQ name
  kBamRnext = 2,     // RNEXT neither "*", "=" nor an @SQ name
  kBamQname = 3,     // QNAME longer than 254 bytes (l_read_name is a byte, NUL included)
  kBamCigarOps = 4,  // more than 65535 CIGAR elements (n_cigar_op is 16 bits)
  kBamPos = 5,       // POS - 1 / PNEXT - 1 / TLEN not an int32
  kBamQual = 6,      // QUAL not "*": a length other than SEQ's, or a byte outside '!'..'~'
  kBamTagType = 7,   // an optional field that is not TG:T:value with T in AifZHB (B: an element type in cCsSiIf)
  kBamIntRange = 8,  // an 'i' value outside [-2^31, 2^32 - 1]
  kBamArrayRange = 9,  // a B value outside its element type
  kBamHex = 10,      // an odd-length or non-hex H
  kBamField = 11,    // FLAG outside [0, 65535] or MAPQ outside [0, 255]
  kBamTagValue = 12, // an A value that is not one byte, an i / f / B value that is not a number
  kBamCodes = 13,
};

struct BamParams {
  const uint8_t* text;
  const uint64_t* line_span;  // [2 n_all]: line start, end (no newline)
  const uint64_t* cig_off;    // the parse's CIGAR words (len << 4 | op: BAM's own encoding)
  const uint32_t* cig;
  const int32_t* sq_id;       // RNAME's @SQ index, -1 none
  samk::NameTable sq;         // RNEXT
  const uint32_t* dup_flags;  // MarkDuplicates' bits in place of FLAG 0x400 (null: the text's)
  int64_t r0, n;              // records [r0, r0 + n)
  uint64_t* len;              // [n] block_size + 4 (pass 1)
  const uint64_t* off;        // [n + 1] exclusive scan (pass 2)
  uint8_t* out;               // the stream (pass 2)
  unsigned long long* err;
  unsigned long long* cnt;    // [0] float values, [1] their text bytes + a NUL each (pass 1); [2], [3] pass 2's cursors
  uint64_t* patch;            // [2 cnt[0]]: stream offset, blob offset
  uint8_t* blob;              // [cnt[1]]
  int64_t cap_patch, cap_blob;
};

// count-or-write byte sink (little endian, unaligned)
struct Out {
  uint8_t* p;  // null: count only
  int64_t n;
  __device__ __forceinline__ void u8(uint32_t v) {
    if (p) p[n] = (uint8_t)v;
    ++n;
  }
  __device__ __forceinline__ void u16(uint32_t v) {
    u8(v & 0xFF);
    u8(v >> 8);
  }
  __device__ __forceinline__ void u32(uint32_t v) {
    u16(v & 0xFFFF);
    u16(v >> 16);
  }
};

// [-+]?[0-9]+ of t[a, b): 0 parsed, 1 not a number, 2 more digits than an int64 holds (out of every range)
__device__ int parse_dec(const uint8_t* t, int64_t a, int64_t b, int64_t* v) {
  bool neg = false;
  if (a < b && (t[a] == '+' || t[a] == '-')) {
    neg = t[a] == '-';
    ++a;
  }
  if (a >= b) return 1;
  for (int64_t i = a; i < b; ++i)
    if (t[i] < '0' || t[i] > '9') return 1;
  while (b - a > 1 && t[a] == '0') ++a;
  if (b - a > 18) return 2;
  int64_t x = 0;
  for (int64_t i = a; i < b; ++i) x = x * 10 + (t[i] - '0');
  *v = neg ? -x : x;
  return 0;
}

// a decimal float strtof consumes whole: [-+]?(digits[.digits*] | .digits)([eE][-+]?digits)? | inf | infinity | nan
__device__ bool float_syntax(const uint8_t* t, int64_t a, int64_t b) {
  if (a < b && (t[a] == '+' || t[a] == '-')) ++a;
  const int64_t n = b - a;
  if (n == 3 || n == 8) {
    const char* w = n == 3 ? ((t[a] | 0x20) == 'i' ? "inf" : "nan") : "infinity";
    int64_t k = 0;
    while (k < n && (t[a + k] | 0x20) == (uint8_t)w[k]) ++k;
    if (k == n) return true;
  }
  int64_t nd = 0;
  while (a < b && t[a] >= '0' && t[a] <= '9') ++a, ++nd;
  if (a < b && t[a] == '.') {
    ++a;
    while (a < b && t[a] >= '0' && t[a] <= '9') ++a, ++nd;
  }
  if (nd == 0) return false;
  if (a < b && (t[a] | 0x20) == 'e') {
    ++a;
    if (a < b && (t[a] == '+' || t[a] == '-')) ++a;
    int64_t ne = 0;
    while (a < b && t[a] >= '0' && t[a] <= '9') ++a, ++ne;
    if (ne == 0) return false;
  }
  return a == b;
}

// element size and range of an integer type letter; false: not one
__device__ __forceinline__ bool int_type(uint8_t ty, int* sz, int64_t* lo, int64_t* hi) {
  switch (ty) {
    case 'c': *sz = 1, *lo = -128, *hi = 127; return true;
    case 'C': *sz = 1, *lo = 0, *hi = 255; return true;
    case 's': *sz = 2, *lo = -32768, *hi = 32767; return true;
    case 'S': *sz = 2, *lo = 0, *hi = 65535; return true;
    case 'i': *sz = 4, *lo = INT32_MIN, *hi = INT32_MAX; return true;
    case 'I': *sz = 4, *lo = 0, *hi = 0xFFFFFFFFll; return true;
    default: return false;
  }
}

// The optional fields t[p, e) in input order.  kWrite: o writes at stream
// offset `base`, float slots go to the patch list; else o counts, *nf / *fb
// take the float values and their text bytes.  Returns kBamOk or the refusal.
template <bool kWrite>
__device__ uint32_t bam_tags(const BamParams& P, int64_t p, int64_t e, Out& o, uint64_t base, uint32_t* nf, uint64_t* fb) {
  const uint8_t* t = P.text;
  auto flt = [&](int64_t a, int64_t b) -> bool {
    if (!float_syntax(t, a, b)) return false;
    if (kWrite) {
      const unsigned long long k = atomicAdd(P.cnt + 2, 1ull);
      const unsigned long long bo = atomicAdd(P.cnt + 3, (unsigned long long)(b - a + 1));
      if ((int64_t)k < P.cap_patch && (int64_t)bo + (b - a + 1) <= P.cap_blob) {  // (pass 1 counted the same walk)
        P.patch[2 * k] = base + (uint64_t)o.n;
        P.patch[2 * k + 1] = bo;
        for (int64_t i = a; i < b; ++i) P.blob[bo + (uint64_t)(i - a)] = t[i];
        P.blob[bo + (uint64_t)(b - a)] = 0;
      }
    } else {
      ++*nf;
      *fb += (uint64_t)(b - a + 1);
    }
    o.u32(0);
    return true;
  };
  for (;;) {
    const int64_t ta = p;
    while (p < e && t[p] != '\t') ++p;
    const int64_t tb = p;
    if (tb - ta < 5 || t[ta + 2] != ':' || t[ta + 4] != ':') return kBamTagType;
    const uint8_t ty = t[ta + 3];
    const int64_t a = ta + 5;
    o.u8(t[ta]);
    o.u8(t[ta + 1]);
    switch (ty) {
      case 'A':
        if (tb - a != 1) return kBamTagValue;
        o.u8('A');
        o.u8(t[a]);
        break;
      case 'i': {
        int64_t v;
        const int rc = parse_dec(t, a, tb, &v);
        if (rc == 1) return kBamTagValue;
        if (rc == 2 || v < INT32_MIN || v > 0xFFFFFFFFll) return kBamIntRange;
        // the smallest type that holds it, signed first (c C s S i I)
        if (v >= -128 && v <= 127) o.u8('c'), o.u8((uint32_t)v & 0xFF);
        else if (v >= 0 && v <= 255) o.u8('C'), o.u8((uint32_t)v);
        else if (v >= -32768 && v <= 32767) o.u8('s'), o.u16((uint32_t)v & 0xFFFF);
        else if (v >= 0 && v <= 65535) o.u8('S'), o.u16((uint32_t)v);
        else if (v <= INT32_MAX) o.u8('i'), o.u32((uint32_t)v);
        else o.u8('I'), o.u32((uint32_t)v);
        break;
      }
      case 'f':
        o.u8('f');
        if (!flt(a, tb)) return kBamTagValue;
        break;
      case 'Z':
        o.u8('Z');
        for (int64_t i = a; i < tb; ++i) o.u8(t[i]);
        o.u8(0);
        break;
      case 'H':
        if ((tb - a) & 1) return kBamHex;
        o.u8('H');
        for (int64_t i = a; i < tb; ++i) {
          const uint8_t c = t[i], l = c | 0x20;
          if (!((c >= '0' && c <= '9') || (l >= 'a' && l <= 'f'))) return kBamHex;
          o.u8(c);
        }
        o.u8(0);
        break;
      case 'B': {
        if (tb - a < 1) return kBamTagType;
        const uint8_t et = t[a];
        int sz = 4;
        int64_t lo = 0, hi = 0;
        const bool is_f = et == 'f';
        if (!is_f && !int_type(et, &sz, &lo, &hi)) return kBamTagType;
        if (tb - a > 1 && t[a + 1] != ',') return kBamTagType;
        uint32_t cnt = 0;
        for (int64_t i = a + 1; i < tb; ++i) cnt += t[i] == ',';
        o.u8('B');
        o.u8(et);
        o.u32(cnt);
        int64_t q = a + 1;
        while (q < tb) {  // t[q] == ','
          const int64_t va = q + 1;
          q = va;
          while (q < tb && t[q] != ',') ++q;
          if (is_f) {
            if (!flt(va, q)) return kBamTagValue;
          } else {
            int64_t v;
            const int rc = parse_dec(t, va, q, &v);
            if (rc == 1) return kBamTagValue;
            if (rc == 2 || v < lo || v > hi) return kBamArrayRange;
            if (sz == 1) o.u8((uint32_t)v & 0xFF);
            else if (sz == 2) o.u16((uint32_t)v & 0xFFFF);
            else o.u32((uint32_t)v);
          }
        }
        break;
      }
      default:
        return kBamTagType;
    }
    if (p >= e) break;
    ++p;
  }
  return kBamOk;
}

struct BamRec {
  int64_t fa[11], fb[11];
  int64_t tags;  // where the optional fields start, -1 none
  int64_t e;
  int64_t flag, pos, mapq, pnext, tlen;  // pos / pnext 0-based
  int32_t ref, nref;
  int64_t n_ops, l_seq;
  bool qual_star;
  int64_t end;  // one past the record's last reference base: pos + the CIGAR's reference length, pos + 1 without one
  uint32_t bin;
  uint32_t code;
};

// the spec's reg2bin (§5.3), arithmetic shifts: beg = -1 falls in bin 4680
__device__ __forceinline__ uint32_t reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}

// fields of record r (index in the parse), validated; x.code: the first refusal in field order
__device__ void bam_fields(const BamParams& P, int64_t r, BamRec& x) {
  const uint8_t* t = P.text;
  const int64_t s = (int64_t)P.line_span[2 * r], e = (int64_t)P.line_span[2 * r + 1];
  int64_t p = s;
  for (int f = 0; f < 11; ++f) {
    x.fa[f] = p;
    while (p < e && t[p] != '\t') ++p;
    x.fb[f] = p;
    if (p < e) ++p;
  }
  x.tags = x.fb[10] < e ? p : -1;
  x.e = e;
  x.code = kBamOk;
  auto bad = [&](uint32_t c) {
    if (x.code == kBamOk) x.code = c;
  };
  auto i32 = [](int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; };
  if (x.fb[0] - x.fa[0] > 254) bad(kBamQname);
  x.flag = x.pos = x.mapq = x.pnext = x.tlen = 0;
  if (!samk::parse_int(t, x.fa[1], x.fb[1], &x.flag)) bad(kBamField);
  if (P.dup_flags) x.flag = (int64_t)adamk::flag_with_dup((uint32_t)x.flag, P.dup_flags[r]);
  if (x.flag < 0 || x.flag > 65535) bad(kBamField);
  const bool rstar = x.fb[2] - x.fa[2] == 1 && t[x.fa[2]] == '*';
  x.ref = rstar ? -1 : P.sq_id[r];
  if (!rstar && x.ref < 0) bad(kBamRname);
  if (!samk::parse_int(t, x.fa[3], x.fb[3], &x.pos) || !i32(--x.pos)) bad(kBamPos);
  if (!samk::parse_int(t, x.fa[4], x.fb[4], &x.mapq) || x.mapq < 0 || x.mapq > 255) bad(kBamField);
  x.n_ops = (int64_t)(P.cig_off[r + 1] - P.cig_off[r]);
  if (x.n_ops > 65535) bad(kBamCigarOps);
  x.nref = adamk::rnext_id(P.sq, t, x.fa[6], x.fb[6], x.ref);
  if (x.nref < 0 && !(x.fb[6] - x.fa[6] == 1 && (t[x.fa[6]] == '*' || t[x.fa[6]] == '='))) bad(kBamRnext);
  if (!samk::parse_int(t, x.fa[7], x.fb[7], &x.pnext) || !i32(--x.pnext)) bad(kBamPos);
  if (!samk::parse_int(t, x.fa[8], x.fb[8], &x.tlen) || !i32(x.tlen)) bad(kBamPos);
  x.l_seq = x.fb[9] - x.fa[9];
  if (x.l_seq == 1 && t[x.fa[9]] == '*') x.l_seq = 0;
  x.qual_star = x.fb[10] - x.fa[10] == 1 && t[x.fa[10]] == '*';
  // reference length: M D N = X
  int64_t ref_len = 0;
  const uint32_t* cg = P.cig + P.cig_off[r];
  for (int64_t k = 0; k < x.n_ops; ++k) {
    const uint32_t op = cg[k] & 15u;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += (int64_t)(cg[k] >> 4);
  }
  x.end = x.pos + (ref_len > 0 ? ref_len : 1);
  x.bin = reg2bin(x.pos, x.end) & 0xFFFFu;
}

// QUAL of a validated record that is not "*": SEQ's length, every byte in '!'..'~'
__device__ bool qual_ok(const uint8_t* t, const BamRec& x) {
  if (x.fb[10] - x.fa[10] != x.l_seq) return false;
  for (int64_t i = x.fa[10]; i < x.fb[10]; ++i)
    if (t[i] < '!' || t[i] > '~') return false;
  return true;
}

// pass 1: every refusal, and block_size + 4
extern "C" __global__ void __launch_bounds__(256) bam_len(BamParams P) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P.n; i += (int64_t)gridDim.x * blockDim.x) {
    BamRec x;
    bam_fields(P, P.r0 + i, x);
    if (x.code == kBamOk && !x.qual_star && !qual_ok(P.text, x)) x.code = kBamQual;
    Out o{nullptr, 0};
    uint32_t nf = 0;
    uint64_t fb = 0;
    if (x.code == kBamOk && x.tags >= 0) x.code = bam_tags<false>(P, x.tags, x.e, o, 0, &nf, &fb);
    if (x.code != kBamOk) atomicMin(P.err, (unsigned long long)(((uint64_t)i << 8) | x.code));
    if (nf) {
      atomicAdd(P.cnt, (unsigned long long)nf);
      atomicAdd(P.cnt + 1, (unsigned long long)fb);
    }
    P.len[i] = (uint64_t)(4 + 32 + (x.fb[0] - x.fa[0] + 1) + 4 * x.n_ops + ((x.l_seq + 1) >> 1) + x.l_seq + o.n);
  }
}

// 4-bit code of a SEQ char: "=ACMGRSVTWYHKDBN", upper-cased, anything else 15
__device__ __forceinline__ uint32_t seq_code(uint8_t c) {
  // letters A..Z by (c & 31) - 1, a nibble each
  constexpr uint64_t kLo = 0xF3FCFFB4FFD2E1ull;       // A B C D E F G H I J K L M N (A in the low nibble)
  constexpr uint64_t kHi = 0xFAF97F865FFFull;         // O P Q R S T U V W X Y Z
  if (c == '=') return 0;
  const uint32_t l = (uint32_t)(c | 0x20) - 'a';
  if (l >= 26) return 15;
  return (uint32_t)((l < 14 ? kLo >> (4 * l) : kHi >> (4 * (l - 14))) & 15u);
}

// pass 2: the bytes.  Whole wavefronts take 64 consecutive records: a lane
// writes its record's fields, name, CIGAR and tags, then the wavefront packs
// SEQ and writes QUAL - 33 of the 64 records one after another, 64 contiguous
// bytes per store instruction.
extern "C" __global__ void __launch_bounds__(256) bam_write(BamParams P) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const uint8_t* t = P.text;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < P.n; i0 += stride) {
    const int64_t i = i0 + lane;
    int64_t seq_a = 0, l_seq = 0, qual_a = -1, dst = 0;
    if (i < P.n) {
      BamRec x;
      const int64_t r = P.r0 + i;
      bam_fields(P, r, x);
      const uint64_t o0 = P.off[i];
      Out o{P.out + o0, 0};
      const int64_t l_name = x.fb[0] - x.fa[0] + 1;
      o.u32((uint32_t)(P.off[i + 1] - o0 - 4));
      o.u32((uint32_t)x.ref);
      o.u32((uint32_t)(int32_t)x.pos);
      o.u8((uint32_t)l_name);
      o.u8((uint32_t)x.mapq);
      o.u16(x.bin);
      o.u16((uint32_t)x.n_ops);
      o.u16((uint32_t)x.flag);
      o.u32((uint32_t)x.l_seq);
      o.u32((uint32_t)x.nref);
      o.u32((uint32_t)(int32_t)x.pnext);
      o.u32((uint32_t)(int32_t)x.tlen);
      for (int64_t k = x.fa[0]; k < x.fb[0]; ++k) o.u8(t[k]);
      o.u8(0);
      const uint32_t* cg = P.cig + P.cig_off[r];
      for (int64_t k = 0; k < x.n_ops; ++k) o.u32(cg[k]);
      seq_a = x.fa[9];
      l_seq = x.l_seq;
      qual_a = x.qual_star ? -1 : x.fa[10];
      dst = (int64_t)o0 + o.n;
      o.n += ((l_seq + 1) >> 1) + l_seq;
      uint32_t nf = 0;
      uint64_t fb = 0;
      if (x.tags >= 0) (void)bam_tags<true>(P, x.tags, x.e, o, o0, &nf, &fb);
    }
    const int live = (int)(P.n - i0 < 64 ? P.n - i0 : 64);
    for (int k = 0; k < live; ++k) {
      const int64_t sa = samk::rl64(seq_a, k), L = samk::rl64(l_seq, k), qa = samk::rl64(qual_a, k);
      uint8_t* d = P.out + samk::rl64(dst, k);
      const int64_t nb = (L + 1) >> 1;
      for (int64_t j = lane; j < nb; j += 64) {
        const uint32_t hi = seq_code(t[sa + 2 * j]);
        const uint32_t lo = 2 * j + 1 < L ? seq_code(t[sa + 2 * j + 1]) : 0u;
        d[j] = (uint8_t)(hi << 4 | lo);
      }
      d += nb;
      for (int64_t j = lane; j < L; j += 64) d[j] = qa < 0 ? (uint8_t)0xFF : (uint8_t)(t[qa + j] - 33);
    }
  }
}

}  // namespace bamo

// the device buffers of the last bqsr_sam_bam_prepare (kept on the parse)
struct BamBufs {
  int64_t r0 = 0, n = 0, cap_n = -1;
  uint64_t *len = nullptr, *off = nullptr, *part = nullptr;
  unsigned long long *err = nullptr, *cnt = nullptr;
  uint8_t* out = nullptr;
  int64_t cap_out = 0, total = 0;
  uint64_t* patch = nullptr;
  uint8_t* blob = nullptr;
  int64_t cap_patch = 0, cap_blob = 0, n_float = 0, blob_bytes = 0;
  StageClock<4> clock;
  bool prepared = false;
  const void *text = nullptr, *spans = nullptr;  // what pass 1 measured: pass 2 runs over the same text only
  void free_rows() {
    for (void* p : {(void*)len, (void*)off, (void*)part})
      if (p) (void)hipFree(p);
    len = off = part = nullptr;
    cap_n = -1;
  }
  ~BamBufs() {
    free_rows();
    for (void* p : {(void*)err, (void*)cnt, (void*)out, (void*)patch, (void*)blob})
      if (p) (void)hipFree(p);
  }
};

namespace {

// pass 1 and pass 2 of the calling thread's last prepare / records or members call, and the clock's marks
enum { BAM_LEN, BAM_WRITE, BAM_STAGES };
enum { BAM_LEN_0, BAM_LEN_1, BAM_WRITE_0, BAM_WRITE_1 };
thread_local double g_bam_ms[BAM_STAGES] = {0.0, 0.0};

const char* kBamErrors[bamo::kBamCodes] = {
    "ok",
    "RNAME is neither '*' nor an @SQ name",
    "RNEXT is neither '*', '=' nor an @SQ name",
    "QNAME longer than 254 bytes",
    "more than 65535 CIGAR elements",
    "POS / PNEXT / TLEN outside int32",
    "QUAL differs from SEQ in length or has a byte outside '!'..'~' (BAM cannot hold the reference's trimmed "
    "recalibrated strings or its chars above 0x7F; the SAM text sink writes them)",
    "an optional field whose type is not one of A i f Z H B (B: of c C s S i I f)",
    "an 'i' tag value outside [-2^31, 2^32 - 1]",
    "a B array value outside its element type",
    "an H tag of odd length or with a non-hex digit",
    "FLAG outside [0, 65535] or MAPQ outside [0, 255]",
    "a tag value that is not of its type (A: one byte; i, f, B: numbers)",
};

bamo::BamParams bam_params(const bqsr_sam* s, const BamBufs& A) {
  bamo::BamParams P{};
  P.text = s->d_text;
  P.line_span = s->line_span;
  P.cig_off = s->cig_off;
  P.cig = s->cig;
  P.sq_id = s->sq_id;
  P.sq = s->sq_tab;
  P.dup_flags = s->dup_marked ? s->flags : nullptr;
  P.r0 = A.r0;
  P.n = A.n;
  P.len = A.len;
  P.off = A.off;
  P.out = A.out;
  P.err = A.err;
  P.cnt = A.cnt;
  P.patch = A.patch;
  P.blob = A.blob;
  P.cap_patch = A.cap_patch;
  P.cap_blob = A.cap_blob;
  return P;
}

// raw DEFLATE for bqsr_bgzf_compress: libdeflate (the system's libdeflate.so.0,
// loaded at run time as bam_ingest.hip's inflate side), zlib otherwise
struct DeflateOut {
  typedef void* (*alloc_fn)(int);
  typedef size_t (*deflate_fn)(void*, const void*, size_t, void*, size_t);
  typedef void (*free_fn)(void*);
  typedef uint32_t (*crc_fn)(uint32_t, const void*, size_t);
  alloc_fn alloc = nullptr;
  deflate_fn deflate = nullptr;
  free_fn free = nullptr;
  crc_fn crc = nullptr;
  static const DeflateOut& get() {
    static const DeflateOut d = [] {
      DeflateOut x;
      const char* off = getenv("ADAM_BQSR_LIBDEFLATE");
      if (off && strcmp(off, "0") == 0) return x;
      void* h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
      if (!h) return x;
      x.alloc = (alloc_fn)dlsym(h, "libdeflate_alloc_compressor");
      x.deflate = (deflate_fn)dlsym(h, "libdeflate_deflate_compress");
      x.free = (free_fn)dlsym(h, "libdeflate_free_compressor");
      x.crc = (crc_fn)dlsym(h, "libdeflate_crc32");
      if (!x.alloc || !x.deflate || !x.free || !x.crc) x = DeflateOut{};
      return x;
    }();
    return d;
  }
  bool ok() const { return alloc != nullptr; }
};

constexpr int64_t kBgzfData = 65280;   // bytes of the stream per member (htslib's BGZF_BLOCK_SIZE - slack)
constexpr int64_t kBgzfSlot = 65536;   // a member's largest size: BSIZE is 16 bits
constexpr int64_t kBgzfFrame = 18 + 8;  // header with the BC field, CRC32 + ISIZE

// One member of `n` (<= kBgzfData) bytes into o (kBgzfSlot bytes); returns its
// size.  level 0, or a DEFLATE stream that would not be smaller: one stored block.
int64_t bgzf_member(const DeflateOut& D, void* comp, int level, const uint8_t* in, int64_t n, uint8_t* o) {
  static const uint8_t kHead[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
  memcpy(o, kHead, 16);
  uint8_t* body = o + 18;
  const int64_t stored = n + 5, avail = kBgzfSlot - kBgzfFrame;
  int64_t c = 0;
  if (level > 0 && n > 0) {
    if (D.ok()) {
      c = (int64_t)D.deflate(comp, in, (size_t)n, body, (size_t)avail);  // 0: it does not fit
    } else {
      z_stream zs{};
      if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK) {
        zs.next_in = (Bytef*)in;
        zs.avail_in = (uInt)n;
        zs.next_out = (Bytef*)body;
        zs.avail_out = (uInt)avail;
        if (deflate(&zs, Z_FINISH) == Z_STREAM_END) c = (int64_t)zs.total_out;
        deflateEnd(&zs);
      }
    }
  }
  if (c <= 0 || c > stored) {  // BFINAL = 1, BTYPE = 00, LEN, ~LEN, the bytes
    body[0] = 1;
    body[1] = (uint8_t)(n & 0xFF);
    body[2] = (uint8_t)(n >> 8);
    body[3] = (uint8_t)(~n & 0xFF);
    body[4] = (uint8_t)((~n >> 8) & 0xFF);
    if (n) memcpy(body + 5, in, (size_t)n);
    c = stored;
  }
  const int64_t size = kBgzfFrame + c;
  o[16] = (uint8_t)((size - 1) & 0xFF);
  o[17] = (uint8_t)((size - 1) >> 8);
  const uint32_t crc = D.ok() ? D.crc(0, in, (size_t)n) : (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, (uInt)n);
  const uint32_t tail[2] = {crc, (uint32_t)n};
  memcpy(body + c, tail, 8);
  return size;
}

// Pass 2 over the prepared range, between its two marks, for both sinks: bqsr_sam_bam_records here and
// bqsr_sam_bam_members (bgzf_deflate.hip).  A sink zeroes the stage with bam_write_begin, runs the pass and,
// after its synchronize, reads the time with bam_write_end.
void bam_write_begin() { g_bam_ms[BAM_WRITE] = 0.0; }

bqsr_status bam_write_pass(bqsr_context* ctx, const bqsr_sam* s, BamBufs& A, hipStream_t st) {
  const bamo::BamParams P = bam_params(s, A);
  HIP_TRY(A.clock.mark(BAM_WRITE_0, st));
  if (A.n > 0) JOB_TRY(launch(bamo::bam_write, sam_grid(A.n, 256, ctx->n_cu * 8), 256, st, P));
  HIP_TRY(A.clock.mark(BAM_WRITE_1, st));
  return BQSR_OK;
}

void bam_write_end(BamBufs& A) { A.clock.add(g_bam_ms[BAM_WRITE], BAM_WRITE_0, BAM_WRITE_1); }

}  // namespace

extern "C" {

bqsr_status bqsr_sam_bam_prepare(bqsr_context* ctx, bqsr_sam* s, int64_t r0, int64_t n, void* stream,
                                 bqsr_bam_sizes* out) {
  if (!ctx || !s || !out || r0 < 0 || n < 0 || r0 + n > s->n_reads)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_bam_prepare: bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = S(stream);
  if (!s->bam) s->bam = std::make_shared<BamBufs>();
  BamBufs& A = *(BamBufs*)s->bam.get();
  A.prepared = false;
  g_bam_ms[BAM_LEN] = g_bam_ms[BAM_WRITE] = 0.0;
  if (A.cap_n < n) {  // per-record buffers, kept across calls
    A.free_rows();
    const size_t N = (size_t)n + 1;
    hipError_t e = hipMalloc((void**)&A.len, N * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&A.off, N * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&A.part, (N / samk::kScanChunk + 2) * 8);
    if (e == hipSuccess && !A.err) e = hipMalloc((void**)&A.err, 8);
    if (e == hipSuccess && !A.cnt) e = hipMalloc((void**)&A.cnt, 4 * 8);
    if (e != hipSuccess) {
      A.free_rows();
      return fail(BQSR_ERR_DEVICE, std::string("bqsr_sam_bam_prepare: ") + hipGetErrorString(e));
    }
    A.cap_n = n;
  }
  A.r0 = r0;
  A.n = n;
  bamo::BamParams P = bam_params(s, A);
  HIP_TRY(hipMemsetAsync(A.err, 0xFF, 8, st));
  HIP_TRY(hipMemsetAsync(A.cnt, 0, 4 * 8, st));
  HIP_TRY(A.clock.mark(BAM_LEN_0, st));
  if (n > 0) JOB_TRY(launch(bamo::bam_len, sam_grid(n, 256, ctx->n_cu * 8), 256, st, P));
  HIP_TRY(A.clock.mark(BAM_LEN_1, st));
  bqsr_status rs = sam_scan(A.len, n, A.off, A.part, st);
  if (rs != BQSR_OK) return rs;
  unsigned long long ew = ~0ull, cnt[2] = {0, 0};
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&ew, A.err, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(cnt, A.cnt, 16, hipMemcpyDeviceToHost, st));
  if (n > 0) HIP_TRY(hipMemcpyAsync(&total, A.off + n, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  A.clock.add(g_bam_ms[BAM_LEN], BAM_LEN_0, BAM_LEN_1);
  if (ew != ~0ull) {
    const uint32_t code = (uint32_t)(ew & 0xFF);
    const int64_t read = r0 + (int64_t)(ew >> 8);
    return fail(BQSR_ERR_UNSUPPORTED,
                "BAM record of read " + std::to_string(read) + ": " + (code < bamo::kBamCodes ? kBamErrors[code] : "?"),
                read);
  }
  A.total = (int64_t)total;
  A.n_float = (int64_t)cnt[0];
  A.blob_bytes = (int64_t)cnt[1];
  auto grow = [](auto** p, int64_t* cap, int64_t want, size_t elem) -> hipError_t {
    if (*cap >= want) return hipSuccess;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const hipError_t e = hipMalloc((void**)p, (size_t)want * elem + 64);
    if (e == hipSuccess) *cap = want;
    return e;
  };
  hipError_t e = grow(&A.out, &A.cap_out, A.total + 1, 1);
  if (e == hipSuccess) e = grow(&A.patch, &A.cap_patch, A.n_float + 1, 16);
  if (e == hipSuccess) e = grow(&A.blob, &A.cap_blob, A.blob_bytes + 1, 1);
  if (e != hipSuccess) return fail(BQSR_ERR_DEVICE, std::string("bqsr_sam_bam_prepare: ") + hipGetErrorString(e));
  out->n_reads = n;
  out->bytes = A.total;
  out->n_floats = A.n_float;
  A.text = s->d_text;
  A.spans = s->line_span;
  A.prepared = true;
  return ok();
}

bqsr_status bqsr_sam_bam_records(bqsr_context* ctx, bqsr_sam* s, uint8_t* dst, void* stream) {
  if (!ctx || !s) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_bam_records: bad arguments");
  BamBufs* Ap = (BamBufs*)s->bam.get();
  if (!Ap || !Ap->prepared) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_bam_records before bqsr_sam_bam_prepare");
  BamBufs& A = *Ap;
  if (A.text != s->d_text || A.spans != s->line_span) {  // rewritten or sorted since: the sizes are stale
    A.prepared = false;
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_bam_records: the text changed since bqsr_sam_bam_prepare");
  }
  if (A.total > 0 && !dst) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_bam_records: no destination");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = S(stream);
  bam_write_begin();
  JOB_TRY(bam_write_pass(ctx, s, A, st));
  std::vector<uint64_t> patch((size_t)A.n_float * 2);
  std::vector<char> blob((size_t)A.blob_bytes + 1, 0);
  if (A.total > 0) HIP_TRY(hipMemcpyAsync(dst, A.out, (size_t)A.total, hipMemcpyDeviceToHost, st));
  if (A.n_float > 0) {
    HIP_TRY(hipMemcpyAsync(patch.data(), A.patch, patch.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(blob.data(), A.blob, (size_t)A.blob_bytes, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  bam_write_end(A);
  // the float slots: strtof of the text pass 2 set aside (correctly rounded, as the C library does it)
  for (int64_t k = 0; k < A.n_float; ++k) {
    const uint64_t at = patch[2 * (size_t)k], bo = patch[2 * (size_t)k + 1];
    if (at + 4 > (uint64_t)A.total || bo >= (uint64_t)A.blob_bytes)
      return fail(BQSR_ERR_DEVICE, "bqsr_sam_bam_records: a float patch outside the stream");
    const float f = strtof(blob.data() + bo, nullptr);
    memcpy(dst + at, &f, 4);
  }
  return ok();
}

bqsr_status bqsr_sam_bam_header(const bqsr_sam* s, uint8_t* dst, int64_t cap, int64_t* len) {
  if (!s || !len || (cap > 0 && !dst)) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_bam_header: bad arguments");
  const std::string& h = s->header_text;
  if (h.size() > (size_t)INT32_MAX) return fail(BQSR_ERR_UNSUPPORTED, "bqsr_sam_bam_header: header text above 2 GiB");
  std::string o("BAM\1", 4);
  auto i32 = [&](int32_t v) { o.append((const char*)&v, 4); };
  i32((int32_t)h.size());
  o += h;
  // every @SQ line in order: l_name, name, NUL, LN (0 when absent)
  std::string refs;
  int32_t n_ref = 0;
  for (size_t p = 0; p < h.size();) {
    size_t e = h.find('\n', p);
    if (e == std::string::npos) e = h.size();
    size_t le = e;
    if (le > p && h[le - 1] == '\r') --le;
    if (le - p >= 3 && h.compare(p, 3, "@SQ") == 0 && (le - p == 3 || h[p + 3] == '\t')) {
      std::string sn;
      int64_t ln = 0;
      bool has_sn = false;
      for (size_t a = p + 3; a < le;) {  // h[a] == '\t'
        size_t b = h.find('\t', a + 1);
        if (b == std::string::npos || b > le) b = le;
        const std::string f = h.substr(a + 1, b - a - 1);
        if (f.compare(0, 3, "SN:") == 0) sn = f.substr(3), has_sn = true;
        else if (f.compare(0, 3, "LN:") == 0) ln = strtoll(f.c_str() + 3, nullptr, 10);
        a = b;
      }
      if (has_sn) {
        const int32_t l_name = (int32_t)sn.size() + 1;
        const int32_t ln32 = (int32_t)std::min<int64_t>(std::max<int64_t>(ln, 0), INT32_MAX);
        refs.append((const char*)&l_name, 4);
        refs += sn;
        refs.push_back('\0');
        refs.append((const char*)&ln32, 4);
        ++n_ref;
      }
    }
    p = e + 1;
  }
  i32(n_ref);
  o += refs;
  *len = (int64_t)o.size();
  if (dst && cap > 0) memcpy(dst, o.data(), (size_t)std::min<int64_t>(cap, *len));
  return ok();
}

bqsr_status bqsr_bgzf_compress(const uint8_t* in, int64_t n, int32_t level, uint8_t* out, int64_t cap,
                               int64_t* out_len) {
  if (n < 0 || (n > 0 && !in) || level < 0 || level > 9 || !out_len || cap < 0 || (cap > 0 && !out))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_bgzf_compress: bad arguments");
  const int64_t nm = (n + kBgzfData - 1) / kBgzfData;
  *out_len = 0;
  if (nm == 0) return ok();
  const DeflateOut& D = DeflateOut::get();
  const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(nm, std::min(16u, std::thread::hardware_concurrency())));
  // members into slots of their largest size, then packed in order
  std::unique_ptr<uint8_t[]> slots(new (std::nothrow) uint8_t[(size_t)(nm * kBgzfSlot)]);
  if (!slots) return fail(BQSR_ERR_DEVICE, "bqsr_bgzf_compress: out of host memory");
  std::vector<int64_t> size((size_t)nm, 0);
  std::atomic<int64_t> next{0};
  std::atomic<bool> failed{false};
  auto work = [&]() {
    void* comp = D.ok() && level > 0 ? D.alloc(level) : nullptr;
    if (D.ok() && level > 0 && !comp) {
      failed = true;
      return;
    }
    for (int64_t m; (m = next.fetch_add(1)) < nm;) {
      const int64_t a = m * kBgzfData;
      size[(size_t)m] = bgzf_member(D, comp, level, in + a, std::min(kBgzfData, n - a), slots.get() + m * kBgzfSlot);
    }
    if (comp) D.free(comp);
  };
  std::vector<std::thread> th;
  for (int k = 1; k < nt; ++k) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  if (failed) return fail(BQSR_ERR_DEVICE, "bqsr_bgzf_compress: no compressor");
  int64_t total = 0;
  for (int64_t v : size) total += v;
  *out_len = total;
  if (total > cap) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bgzf_compress: the output does not fit (see *out_len)");
  int64_t at = 0;
  for (int64_t m = 0; m < nm; ++m) {
    memcpy(out + at, slots.get() + m * kBgzfSlot, (size_t)size[(size_t)m]);
    at += size[(size_t)m];
  }
  return ok();
}

bqsr_status bqsr_bam_kernel_times(double* len_ms, double* write_ms) {
  if (len_ms) *len_ms = g_bam_ms[BAM_LEN];
  if (write_ms) *write_ms = g_bam_ms[BAM_WRITE];
  return ok();
}

}  // extern "C"
