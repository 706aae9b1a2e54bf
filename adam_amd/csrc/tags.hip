// `adam print_tags` on the device (include/adam_sam.h: bqsr_sam_tag_counts,
// bqsr_arrow_tag_counts, bqsr_sam_tag_values, bqsr_arrow_tag_values):
// adamCharacterizeTags / adamCharacterizeTagValues
// (core/rdd/AdamRDDFunctions.scala:200-229) over RichADAMRecord.tags
// (core/rich/RichADAMRecord.scala:46) of the records cli/PrintTags.scala:70
// keeps (!failedVendorQualityChecks).
//
// One scanning core, two front ends.  The core validates one attribute as
// AttributeUtils.parseAttribute would (core/util/AttributeUtils.scala:28-99)
// and adds its tag to the histogram.
//
//   check_piece   the whole piece matches ([^:]{2}):([AifZHB]):(.*)
//       (AttributeUtils.scala:28,59-66; Java's `.` stops at \n, \r, U+0085,
//       U+2028, U+2029), then typedStringToValue (:87-99): A valueStr(0), i
//       Integer.valueOf, f Float.valueOf, Z the string, H a Byte.valueOf per
//       char, B split(",") into Float.valueOf / Integer.valueOf.  What throws
//       is kAttr (BQSR_ERR_ATTRIBUTE).  A tag byte >= 0x80, or one inside an
//       A / i / f / H / B value, is kUnsup: the regex counts UTF-16 chars and
//       Java's number parsers take non-ASCII digits, neither restated here.
//   hist_add      a workgroup owns a 95 x 95 table of u32 in LDS (36 100 B, so
//       four workgroups share a CU's 160 KB) indexed by the two tag bytes in
//       0x20..0x7E.  The lanes of a wavefront walk their records' k-th
//       attribute in lockstep and nearly every read carries the same dozen
//       tags, so the adds of a step are aggregated: the first pending lane's
//       bin is broadcast, a ballot finds the lanes holding the same bin, the
//       leader adds the popcount once, and the loop goes on with the lanes
//       left (once or twice for real files).  Tag bytes below 0x20 or 0x7F
//       (legal for the regex) go straight to the global table.  A workgroup
//       meets fewer than 2^32 records of one parse, so no bin can wrap.  At the
//       end of the grid-stride loop each non-zero bin is one 64-bit atomicAdd
//       into the 128 x 128 table (first byte * 128 + second byte).  Integer
//       sums: nothing depends on the launch order.
//   tags_scan_sam    a lane per record of a parse.  The tags are collected by
//       adam_out.hip's collect_tags / attributes_text -- htsjdk's sorted list,
//       a repeat replaced, MD left out, and the converter's errors (H / B, an
//       `i` outside Int, an unparsable i / f, more than 48 tags) -- for every
//       record; the records with FLAG 0x200 clear are then checked tag by tag
//       as the converter would have printed them (SAMRecordConverter.scala:
//       110-121: descending binary tag) and counted.
//   tags_scan_arrow  a lane per record of one Arrow chunk: the attributes
//       column (int32 offsets, bytes, validity) and the
//       failedVendorQualityChecks bitmap.  A null failedVendorQualityChecks,
//       or null attributes on a kept record, is kNull (PrintTags.scala:70
//       unboxes null; parseAttributes(null) :47).  The string is split on
//       tabs, empty pieces dropped (:48), every piece checked and counted.
//
// The kept records are counted by ballot + popcount beside the histogram.
// Errors: one atomicMin word (record << 8 | code), so the first failing record
// in input order wins; a lane reports its record's first error only --
// conversion errors, then kNull, then the first bad attribute in string order.
//
// -count, one tag T a call (adamCharacterizeTagValues, AdamRDDFunctions.scala:
// 211-219: the value of the first attribute tagged T of every record that has
// one, counted per distinct value):
//   tag_value_keys   a lane per record: a 64-bit key -- the type (A i f Z H)
//       in the top three bits over the scalar (i: the int, f: floatToIntBits
//       with one NaN, A: the byte) or over a 56-bit FNV-1a of the value bytes
//       cut to hash_bits (Z, H) -- the value's span, and a has-flag; a scan of
//       the flags compacts (key, record) into input order (tag_value_compact)
//   rocprim::radix_sort_pairs, stable: equal keys stay in input order
//   tag_value_heads  a run starts where the key differs from the element
//       before it or, for Z / H, where the bytes differ: a hash collision
//       splits a run and never merges two values
//   tag_value_runs / tag_value_text  per run: type, length, first record, and
//       the value's text (decimal, samk::java_float_text, or the bytes)
// The host merges runs by (type, text), so counts are exact whatever the hash
// does.  A first attribute of type B is kValueB (BQSR_ERR_UNSUPPORTED): its
// value is a Java array keyed by identity.  The value kernels do not validate:
// callers run the scan over the same records first.
//
// Included by bqsr_capi.cpp after compare.hip (collect_tags, attributes_text,
// sam_alloc, sam_scan and SortTmp come from the files before it).

namespace tagk {

constexpr int kThreads = 256;
constexpr int kSide = 95;                 // tag bytes 0x20..0x7E
constexpr int kBins = kSide * kSide;      // the LDS table
constexpr int kTable = 128 * 128;         // the global table
constexpr int kTotal = kTable, kErr = kTable + 1, kWords = kTable + 2;

// error codes behind adam_out.hip's kAdam* (1..4)
enum : uint32_t { kNull = 5, kAttr = 6, kUnsup = 7, kOffsets = 8, kValueB = 9 };

__device__ __forceinline__ bool bit(const uint8_t* bm, int64_t i) { return (bm[i >> 3] >> (i & 7)) & 1u; }

// does Java's `.` stop inside t[a, b)?  \n, \r, U+0085 (C2 85), U+2028 / U+2029 (E2 80 A8 / A9)
__device__ bool has_line_end(const uint8_t* t, int64_t a, int64_t b) {
  for (int64_t i = a; i < b; ++i) {
    const uint8_t c = t[i];
    if (c == '\n' || c == '\r') return true;
    if (c == 0xC2 && i + 1 < b && t[i + 1] == 0x85) return true;
    if (c == 0xE2 && i + 2 < b && t[i + 1] == 0x80 && (t[i + 2] == 0xA8 || t[i + 2] == 0xA9)) return true;
  }
  return false;
}

// Integer.valueOf (Java 7+: an optional '+' or '-', decimal digits, within Int)
__device__ bool java_int(const uint8_t* t, int64_t a, int64_t b, int32_t* v) {
  bool neg = false;
  if (a < b && (t[a] == '+' || t[a] == '-')) {
    neg = t[a] == '-';
    ++a;
  }
  if (a >= b) return false;
  int64_t x = 0;
  for (int64_t i = a; i < b; ++i) {
    if (t[i] < '0' || t[i] > '9') return false;
    x = x * 10 + (t[i] - '0');
    if (x > 2147483648ll) x = 2147483649ll;  // (stays too large)
  }
  if (x > (neg ? 2147483648ll : 2147483647ll)) return false;
  *v = (int32_t)(neg ? -x : x);
  return true;
}

// Float.valueOf of t[a, b): 0, kAttr, or kUnsup for a hexadecimal float (Java takes it; not restated here)
__device__ uint32_t check_float(const uint8_t* t, int64_t a, int64_t b) {
  float fv;
  if (samk::java_parse_float(t, a, b, &fv)) return 0;
  while (a < b && t[a] <= ' ') ++a;
  if (a < b && (t[a] == '+' || t[a] == '-')) ++a;
  return a + 1 < b && t[a] == '0' && (t[a + 1] == 'x' || t[a + 1] == 'X') ? kUnsup : kAttr;
}

// typedStringToValue of a value the regex's (.*) would take (AttributeUtils.scala:87-99): 0, kAttr or kUnsup
__device__ uint32_t check_value(const uint8_t* t, uint8_t type, int64_t a, int64_t b) {
  if (has_line_end(t, a, b)) return kAttr;
  if (type == 'Z') return 0;
  for (int64_t i = a; i < b; ++i)
    if (t[i] >= 0x80) return kUnsup;
  int32_t iv;
  switch (type) {
    case 'A':
      return a < b ? 0 : kAttr;
    case 'i':
      return java_int(t, a, b, &iv) ? 0 : kAttr;
    case 'f':
      return check_float(t, a, b);
    case 'H':
      for (int64_t i = a; i < b; ++i)
        if (t[i] < '0' || t[i] > '9') return kAttr;  // Byte.valueOf("" + c)
      return 0;
    default: {  // 'B': split(",") drops trailing empty strings; "" stays one empty piece
      if (a == b) return kAttr;
      while (b > a && t[b - 1] == ',') --b;
      while (a < b) {
        int64_t e = a;
        bool dot = false;
        while (e < b && t[e] != ',') dot = dot || t[e] == '.', ++e;
        const uint32_t c = dot ? check_float(t, a, e) : java_int(t, a, e, &iv) ? 0u : (uint32_t)kAttr;
        if (c) return c;
        a = e + 1;
      }
      return 0;
    }
  }
}

// parseAttribute of the piece t[a, b) (not empty): 0 with *id = the binary tag, kAttr or kUnsup
__device__ uint32_t check_piece(const uint8_t* t, int64_t a, int64_t b, uint32_t* id) {
  const int64_t n = b - a;
  if (t[a] >= 0x80 || (n >= 2 && t[a + 1] >= 0x80)) return kUnsup;
  if (n < 5 || t[a] == ':' || t[a + 1] == ':' || t[a + 2] != ':' || t[a + 4] != ':') return kAttr;
  const uint8_t ty = t[a + 3];
  if (ty != 'A' && ty != 'i' && ty != 'f' && ty != 'Z' && ty != 'H' && ty != 'B') return kAttr;
  *id = (uint32_t)t[a] | ((uint32_t)t[a + 1] << 8);
  return check_value(t, ty, a + 5, b);
}

// a tag the converter converted, as it prints it ("%s:%s:%s"): i and f values
// are its own decimal / Float.toString text, A and Z values the line's bytes
__device__ uint32_t check_sam_tag(const uint8_t* t, const adamk::Tag& g) {
  const uint32_t b0 = g.id & 0xFF, b1 = g.id >> 8;
  if (b0 >= 0x80 || b1 >= 0x80) return kUnsup;
  if (b0 == ':' || b1 == ':') return kAttr;
  return g.type == 'A' || g.type == 'Z' ? check_value(t, g.type, g.a, g.b) : 0;
}

// one step of a wavefront: the lanes with `have` add 1 at their tag (all lanes call)
__device__ __forceinline__ void hist_add(uint32_t* bins, unsigned long long* table, bool have, uint32_t id,
                                         int lane) {
  const uint32_t b0 = id & 0xFF, b1 = (id >> 8) & 0xFF;
  const bool dense = have && b0 - 0x20u < (uint32_t)kSide && b1 - 0x20u < (uint32_t)kSide;
  if (have && !dense) atomicAdd(&table[(b0 & 127u) * 128u + (b1 & 127u)], 1ull);  // the rare path
  const uint32_t bin = dense ? (b0 - 0x20u) * kSide + (b1 - 0x20u) : 0u;
  uint64_t todo = __builtin_amdgcn_ballot_w64(dense);
  while (todo) {  // (uniform)
    const int leader = __builtin_ctzll(todo);
    const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
    const uint64_t same = __builtin_amdgcn_ballot_w64(dense && bin == lb);
    if (lane == leader) atomicAdd(&bins[lb], (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

__device__ __forceinline__ void bins_clear(uint32_t* bins) {
  for (int j = threadIdx.x; j < kBins; j += kThreads) bins[j] = 0;
  __syncthreads();
}
__device__ __forceinline__ void bins_flush(const uint32_t* bins, unsigned long long* table) {
  __syncthreads();
  for (int j = threadIdx.x; j < kBins; j += kThreads) {
    const uint32_t v = bins[j];
    if (v) atomicAdd(&table[(j / kSide + 0x20) * 128 + (j % kSide + 0x20)], (unsigned long long)v);
  }
}

// where the optional fields of record i start -- behind the QUAL field the
// parse recorded (the eleventh; the parse saw eleven) -- and whether there are any
__device__ __forceinline__ int64_t tags_start(const uint64_t* qual_span, int64_t i, int64_t e, bool* more) {
  const int64_t q = (int64_t)qual_span[2 * i + 1];
  *more = q < e;
  return q < e ? q + 1 : e;
}

// out: [kTable] counts, the kept records, the error word
extern "C" __global__ void __launch_bounds__(kThreads) tags_scan_sam(const uint8_t* __restrict__ text,
                                                                     const uint64_t* __restrict__ line_span,
                                                                     const uint64_t* __restrict__ qual_span,
                                                                     const uint32_t* __restrict__ raw_flag, int64_t n,
                                                                     unsigned long long* out) {
  __shared__ uint32_t bins[kBins];
  bins_clear(bins);
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  adamk::Tag tg[adamk::kMaxTags];
  unsigned long long kept = 0;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < n; i0 += stride) {
    const int64_t i = i0 + lane;
    int k = -1;
    uint32_t err = 0;
    bool keep = false;
    if (i < n) {
      const int64_t e = (int64_t)line_span[2 * i + 1];
      bool more;
      const int64_t p = tags_start(qual_span, i, e, &more);
      uint32_t code;
      const int nt = adamk::collect_tags(text, p, e, more, tg, &code);
      if (code == adamk::kAdamOk) (void)adamk::attributes_text(text, tg, nt, nullptr, &code);
      err = code;
      keep = !err && !(raw_flag[i] & 0x200u);  // FLAG 0: failedVendorQualityChecks false (quirk Q2)
      if (keep) k = nt - 1;
    }
    kept += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(keep));
    for (; __builtin_amdgcn_ballot_w64(k >= 0); --k) {  // the k-th attribute of the string, in lockstep
      bool have = false;
      uint32_t id = 0;
      if (k >= 0 && tg[k].id != adamk::kTagMD) {
        err = check_sam_tag(text, tg[k]);
        have = !err;
        id = tg[k].id;
        if (err) k = -1;
      }
      hist_add(bins, out, have, id, lane);
    }
    if (err) atomicMin(&out[kErr], (unsigned long long)(((uint64_t)i << 8) | err));
  }
  if (lane == 0 && kept) atomicAdd(&out[kTotal], kept);
  bins_flush(bins, out);
}

// One Arrow chunk on the device: the attributes column (off null: every
// record's attributes null) and failedVendorQualityChecks (failed null: every
// value null).  off[i] - off_base is record i's start in bytes[0, n_bytes).
struct ArrowTags {
  const int32_t* off;
  const uint8_t* bytes;
  const uint8_t* valid;
  const uint8_t* failed;
  const uint8_t* failed_valid;
  int64_t off_base, n_bytes, n, base;
};

// record i of the chunk: kept (not failed), its attributes' span; 0 or the error
__device__ __forceinline__ uint32_t arrow_record(const ArrowTags& C, int64_t i, bool* keep, int64_t* a, int64_t* b) {
  *keep = false;
  *a = *b = 0;
  if (!C.failed || (C.failed_valid && !bit(C.failed_valid, i))) return kNull;
  if (bit(C.failed, i)) return 0;
  if (!C.off || (C.valid && !bit(C.valid, i))) return kNull;
  const int64_t x = (int64_t)C.off[i] - C.off_base, y = (int64_t)C.off[i + 1] - C.off_base;
  if (x < 0 || y < x || y > C.n_bytes) return kOffsets;
  *keep = true;
  *a = x;
  *b = y;
  return 0;
}

extern "C" __global__ void __launch_bounds__(kThreads) tags_scan_arrow(ArrowTags C, unsigned long long* out) {
  __shared__ uint32_t bins[kBins];
  bins_clear(bins);
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const uint8_t* t = C.bytes;
  unsigned long long kept = 0;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < C.n; i0 += stride) {
    const int64_t i = i0 + lane;
    uint32_t err = 0;
    bool keep = false;
    int64_t p = 0, e = 0;
    if (i < C.n) err = arrow_record(C, i, &keep, &p, &e);
    kept += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(keep));
    bool more = keep && p < e;
    while (__builtin_amdgcn_ballot_w64(more)) {  // the next piece that is not empty, in lockstep
      bool have = false;
      uint32_t id = 0;
      if (more) {
        while (p < e && t[p] == '\t') ++p;
        if (p < e) {
          const int64_t a = p;
          while (p < e && t[p] != '\t') ++p;
          err = check_piece(t, a, p, &id);
          have = !err;
        }
        more = !err && p < e;
      }
      hist_add(bins, out, have, id, lane);
    }
    if (err) atomicMin(&out[kErr], (unsigned long long)(((uint64_t)(C.base + i) << 8) | err));
  }
  if (lane == 0 && kept) atomicAdd(&out[kTotal], kept);
  bins_flush(bins, out);
}

// ---- -count ----

// the records of a values call: a parse (line_span set) or an Arrow chunk
struct Values {
  const uint8_t* text;  // the parse's text, or the chunk's bytes
  const uint64_t* line_span;
  const uint64_t* qual_span;
  const uint32_t* raw_flag;
  ArrowTags C;
  int64_t n;
  uint32_t tag;  // binary tag
  int bits;      // hash width
};

constexpr int kTypeShift = 61;
constexpr uint64_t kHashMask = (1ull << 56) - 1ull;
__device__ __forceinline__ int type_index(uint8_t ty) {
  return ty == 'A' ? 0 : ty == 'i' ? 1 : ty == 'f' ? 2 : ty == 'Z' ? 3 : ty == 'H' ? 4 : 5;
}

// the value record i contributes: its type and span (false: none)
__device__ bool first_value(const Values& V, int64_t i, adamk::Tag* tg, uint8_t* type, int64_t* a, int64_t* b) {
  const uint8_t* t = V.text;
  if (V.line_span) {  // the surviving tag of the line
    if (V.raw_flag[i] & 0x200u || V.tag == adamk::kTagMD) return false;
    const int64_t e = (int64_t)V.line_span[2 * i + 1];
    bool more;
    const int64_t p = tags_start(V.qual_span, i, e, &more);
    uint32_t code;
    const int nt = adamk::collect_tags(t, p, e, more, tg, &code);
    for (int k = 0; k < nt; ++k)
      if (tg[k].id == V.tag) {
        *type = tg[k].type;
        *a = tg[k].a;
        *b = tg[k].b;
        return true;
      }
    return false;
  }
  bool keep;
  int64_t p, e;
  if (arrow_record(V.C, i, &keep, &p, &e) || !keep) return false;
  while (p < e) {  // the first piece tagged T
    while (p < e && t[p] == '\t') ++p;
    const int64_t x = p;
    while (p < e && t[p] != '\t') ++p;
    if (p - x >= 5 && ((uint32_t)t[x] | ((uint32_t)t[x + 1] << 8)) == V.tag) {
      *type = t[x + 3];
      *a = x + 5;
      *b = p;
      return true;
    }
  }
  return false;
}

extern "C" __global__ void __launch_bounds__(kThreads) tag_value_keys(Values V, uint64_t* key, uint64_t* has,
                                                                      int64_t* va, uint32_t* vlen,
                                                                      unsigned long long* err) {
  adamk::Tag tg[adamk::kMaxTags];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < V.n; i += (int64_t)gridDim.x * blockDim.x) {
    uint8_t ty = 0;
    int64_t a = 0, b = 0;
    bool ok = first_value(V, i, tg, &ty, &a, &b);
    uint64_t k = 0;
    if (ok) {
      const int ti = type_index(ty);
      int32_t iv = 0;
      float fv;
      if (ti == 0) {
        ok = a < b;
        if (ok) k = V.text[a];
      } else if (ti == 1) {
        ok = java_int(V.text, a, b, &iv);
        k = (uint32_t)iv;
      } else if (ti == 2) {
        ok = samk::java_parse_float(V.text, a, b, &fv);
        k = fv != fv ? 0x7fc00000u : __float_as_uint(fv);  // floatToIntBits: one NaN
      } else if (ti <= 4) {
        uint64_t h = samk::fnv1a(V.text + a, b - a);
        if (V.bits < 64) h &= (1ull << V.bits) - 1ull;
        k = h & kHashMask;
      } else {
        ok = false;
        if (ty == 'B') atomicMin(err, (unsigned long long)(((uint64_t)(V.C.base + i) << 8) | kValueB));
      }
      k |= (uint64_t)ti << kTypeShift;
    }
    key[i] = k;
    has[i] = ok ? 1ull : 0ull;
    va[i] = a;
    vlen[i] = (uint32_t)(b - a);
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) tag_value_compact(const uint64_t* key, const uint64_t* has,
                                                                         const uint64_t* off, int64_t n, uint64_t* ck,
                                                                         uint32_t* ci) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (has[i]) {
      ck[off[i]] = key[i];
      ci[off[i]] = (uint32_t)i;
    }
}

extern "C" __global__ void __launch_bounds__(kThreads) tag_value_heads(const uint8_t* text, const uint64_t* ck,
                                                                       const uint32_t* ci, const int64_t* va,
                                                                       const uint32_t* vlen, int64_t m,
                                                                       uint64_t* head) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    bool h = j == 0 || ck[j] != ck[j - 1];
    if (!h && (ck[j] >> kTypeShift) >= 3) {  // Z / H: the bytes decide
      const uint32_t r = ci[j], q = ci[j - 1];
      h = vlen[r] != vlen[q];
      for (uint32_t x = 0; !h && x < vlen[r]; ++x) h = text[va[r] + x] != text[va[q] + x];
    }
    head[j] = h ? 1ull : 0ull;
  }
}

// the text of the value behind key k (out null: its length)
__device__ int64_t value_text(const uint8_t* text, uint64_t k, int64_t a, uint32_t len, uint8_t* out) {
  const int ti = (int)(k >> kTypeShift);
  if (ti == 0) {
    if (out) out[0] = (uint8_t)k;
    return 1;
  }
  if (ti == 1) {
    bamk::Put p{out, 0};
    p.integer((int64_t)(int32_t)(uint32_t)k);
    return p.n;
  }
  if (ti == 2) return samk::java_float_text(__uint_as_float((uint32_t)k), out);
  if (out)
    for (uint32_t x = 0; x < len; ++x) out[x] = text[a + x];
  return len;
}

extern "C" __global__ void __launch_bounds__(kThreads) tag_value_runs(const uint8_t* text, const uint64_t* ck,
                                                                      const uint32_t* ci, const int64_t* va,
                                                                      const uint32_t* vlen, const uint64_t* head,
                                                                      const uint64_t* rid, int64_t m, uint64_t* rpos,
                                                                      uint64_t* rlen) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x)
    if (head[j]) {
      const uint32_t r = ci[j];
      rpos[rid[j]] = (uint64_t)j;
      rlen[rid[j]] = (uint64_t)value_text(text, ck[j], va[r], vlen[r], nullptr);
    }
}

extern "C" __global__ void __launch_bounds__(kThreads) tag_value_text(const uint8_t* text, const uint64_t* ck,
                                                                      const uint32_t* ci, const int64_t* va,
                                                                      const uint32_t* vlen, const uint64_t* rpos,
                                                                      const uint64_t* toff, int64_t nr, int64_t m,
                                                                      int64_t base, uint8_t* rtype, int64_t* rcount,
                                                                      int64_t* rfirst, uint8_t* out) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nr; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = (int64_t)rpos[r], j1 = r + 1 < nr ? (int64_t)rpos[r + 1] : m;
    const uint32_t rec = ci[j];  // (stable sort: the run's first record in input order)
    const char kLetters[] = "AifZH";
    rtype[r] = (uint8_t)kLetters[ck[j] >> kTypeShift];
    rcount[r] = j1 - j;
    rfirst[r] = base + rec;
    (void)value_text(text, ck[j], va[rec], vlen[rec], out + toff[r]);
  }
}

}  // namespace tagk

namespace {

// the scan kernels of the calling thread's last counts call, the value kernels (with their sorts and scans) of its
// last values call; either call times its work between the two marks of a clock of its own
enum { TAGS_SCAN, TAGS_VALUES, TAGS_STAGES };
thread_local double g_tags_ms[TAGS_STAGES] = {0.0, 0.0};
typedef StageClock<2> TagClock;

// the runs of the last bqsr_*_tag_values call of this thread
struct TagRuns {
  std::vector<uint8_t> type, text;
  std::vector<int64_t> count, first, toff{0};
  void clear() {
    type.clear();
    text.clear();
    count.clear();
    first.clear();
    toff.assign(1, 0);
  }
};
thread_local TagRuns g_tag_runs;

// at most four workgroups a CU (their LDS tables), or BQSR_TUNE_FLAGSTAT_GRID in all
unsigned tags_grid(const bqsr_context* ctx, int64_t n) {
  return sam_grid(n, tagk::kThreads, ctx->tune_flagstat_grid > 0 ? ctx->tune_flagstat_grid : ctx->n_cu * 4);
}

bqsr_status tags_block(SortTmp& T, unsigned long long** d, hipStream_t s) {
  bqsr_status e;
  if ((e = sam_alloc(T.v, d, (size_t)tagk::kWords)) != BQSR_OK) return e;
  HIP_TRY(hipMemsetAsync(*d, 0, tagk::kErr * 8, s));
  HIP_TRY(hipMemsetAsync(*d + tagk::kErr, 0xFF, 8, s));
  return BQSR_OK;
}

bqsr_status tags_error(unsigned long long w) {
  const uint32_t code = (uint32_t)(w & 0xFF);
  const int64_t read = (int64_t)(w >> 8);
  const std::string r = "print_tags: read " + std::to_string(read);
  switch (code) {
    case tagk::kNull:
      return fail(BQSR_ERR_NULL_FIELD,
                  r + " has a null failedVendorQualityChecks or null attributes (the reference throws a "
                      "NullPointerException)",
                  read);
    case tagk::kAttr:
      return fail(BQSR_ERR_ATTRIBUTE, r + " has an attribute AttributeUtils.parseAttribute throws at", read);
    case tagk::kUnsup:
      return fail(BQSR_ERR_UNSUPPORTED,
                  r + " has a non-ASCII byte in a tag name or in an A / i / f / H / B value", read);
    case tagk::kOffsets:
      return fail(BQSR_ERR_INVALID_ARG, r + ": the attributes offsets leave the column's bytes", read);
    case tagk::kValueB:
      return fail(BQSR_ERR_UNSUPPORTED,
                  r + ": the counted tag's value is of type B (an array the reference keys by identity)", read);
    default:
      return adam_code_fail(code, read);
  }
}

bqsr_status tags_finish(unsigned long long* d, hipStream_t s, TagClock& clock, bqsr_tag_counts* out) {
  std::vector<unsigned long long> h((size_t)tagk::kWords);
  HIP_TRY(hipMemcpyAsync(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  clock.add(g_tags_ms[TAGS_SCAN], 0, 1);
  if (h[tagk::kErr] != ~0ull) return tags_error(h[tagk::kErr]);
  for (int k = 0; k < tagk::kTable; ++k) out->counts[k] = (int64_t)h[k];
  out->total = (int64_t)h[tagk::kTotal];
  return ok();
}

// an Arrow chunk's buffers on the device (staging owned by T)
bqsr_status tags_stage(SortTmp& T, const bqsr_tags_chunk& H, int64_t base, hipStream_t s, tagk::ArrowTags* C) {
  *C = tagk::ArrowTags{};
  const int64_t m = H.n_reads;
  C->n = m;
  C->base = base;
  const size_t vb = (size_t)(m + 7) / 8;
  bqsr_status e;
  auto bitmap = [&](const uint8_t* src, const uint8_t** dst) -> bqsr_status {
    uint8_t* d;
    if (!src) return BQSR_OK;
    if ((e = sam_alloc(T.v, &d, vb)) != BQSR_OK) return e;
    HIP_TRY(hipMemcpyAsync(d, src, vb, hipMemcpyHostToDevice, s));
    *dst = d;
    return BQSR_OK;
  };
  if ((e = bitmap(H.failed, &C->failed)) || (e = bitmap(H.failed ? H.failed_validity : nullptr, &C->failed_valid)))
    return e;
  if (H.attr_offsets) {
    const int64_t lo = H.attr_offsets[0], hi = H.attr_offsets[m];
    if (lo < 0 || hi < lo || (hi > lo && !H.attr_bytes))
      return fail(BQSR_ERR_INVALID_ARG, "print_tags: bad attributes offsets");
    int32_t* d_off;
    uint8_t* d_bytes;
    if ((e = sam_alloc(T.v, &d_off, (size_t)m + 1)) || (e = sam_alloc(T.v, &d_bytes, (size_t)(hi - lo)))) return e;
    HIP_TRY(hipMemcpyAsync(d_off, H.attr_offsets, ((size_t)m + 1) * 4, hipMemcpyHostToDevice, s));
    if (hi > lo) HIP_TRY(hipMemcpyAsync(d_bytes, H.attr_bytes + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, s));
    C->off = d_off;
    C->bytes = d_bytes;
    C->off_base = lo;
    C->n_bytes = hi - lo;
    if ((e = bitmap(H.attr_validity, &C->valid))) return e;
  }
  return BQSR_OK;
}

bqsr_status tags_chunks_ok(const bqsr_tags_chunk* chunks, int32_t n_chunks, const char* who) {
  if (n_chunks < 0 || (n_chunks && !chunks)) return fail(BQSR_ERR_INVALID_ARG, std::string(who) + ": bad arguments");
  for (int32_t c = 0; c < n_chunks; ++c)
    if (chunks[c].n_reads < 0 || chunks[c].n_reads > INT32_MAX)
      return fail(BQSR_ERR_INVALID_ARG, std::string(who) + ": a chunk length outside 0 .. 2^31 - 1");
  return BQSR_OK;
}

// the runs of V's values appended to g_tag_runs; V.C.base = the global index of record 0
bqsr_status tag_values_run(bqsr_context* ctx, tagk::Values V, hipStream_t s) {
  const int64_t n = V.n;
  if (n == 0) return BQSR_OK;
  if (n > 0xFFFFFFFFll) return fail(BQSR_ERR_UNSUPPORTED, "print_tags: more than 2^32 - 1 records in one call");
  SortTmp T;
  bqsr_status e;
  const size_t N = (size_t)n;
  uint64_t *key, *has, *off, *part;
  int64_t* va;
  uint32_t* vlen;
  unsigned long long* err;
  if ((e = sam_alloc(T.v, &key, N)) || (e = sam_alloc(T.v, &has, N)) || (e = sam_alloc(T.v, &off, N + 1)) ||
      (e = sam_alloc(T.v, &part, N / samk::kScanChunk + 2)) || (e = sam_alloc(T.v, &va, N)) ||
      (e = sam_alloc(T.v, &vlen, N)) || (e = sam_alloc(T.v, &err, 1)))
    return e;
  HIP_TRY(hipMemsetAsync(err, 0xFF, 8, s));
  const unsigned g = sam_grid(n, tagk::kThreads, ctx->n_cu * 8);
  JOB_TRY(launch(tagk::tag_value_keys, g, tagk::kThreads, s, V, key, has, va, vlen, err));
  if ((e = sam_scan(has, n, off, part, s)) != BQSR_OK) return e;
  unsigned long long ew = ~0ull;
  uint64_t m64 = 0;
  HIP_TRY(hipMemcpyAsync(&ew, err, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&m64, off + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (ew != ~0ull) return tags_error(ew);
  const int64_t m = (int64_t)m64;
  if (m == 0) return BQSR_OK;
  const size_t M = (size_t)m;
  uint64_t *ck, *ck2, *head, *rid, *rpos, *rlen, *toff;
  uint32_t *ci, *ci2;
  if ((e = sam_alloc(T.v, &ck, M)) || (e = sam_alloc(T.v, &ck2, M)) || (e = sam_alloc(T.v, &ci, M)) ||
      (e = sam_alloc(T.v, &ci2, M)) || (e = sam_alloc(T.v, &head, M)) || (e = sam_alloc(T.v, &rid, M + 1)))
    return e;
  JOB_TRY(launch(tagk::tag_value_compact, g, tagk::kThreads, s, key, has, off, n, ck, ci));
  if ((e = with_temp(T.v, [&](void* t, size_t& b) {
         return rocprim::radix_sort_pairs(t, b, ck, ck2, ci, ci2, M, 0, 64, s);
       })))
    return e;
  const unsigned gm = sam_grid(m, tagk::kThreads, ctx->n_cu * 8);
  JOB_TRY(launch(tagk::tag_value_heads, gm, tagk::kThreads, s, V.text, ck2, ci2, va, vlen, m, head));
  if ((e = sam_scan(head, m, rid, part, s)) != BQSR_OK) return e;
  uint64_t nr64 = 0;
  HIP_TRY(hipMemcpyAsync(&nr64, rid + m, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int64_t nr = (int64_t)nr64;
  const size_t R = (size_t)nr;
  uint8_t* rtype;
  int64_t *rcount, *rfirst;
  if ((e = sam_alloc(T.v, &rpos, R)) || (e = sam_alloc(T.v, &rlen, R)) || (e = sam_alloc(T.v, &toff, R + 1)) ||
      (e = sam_alloc(T.v, &rtype, R)) || (e = sam_alloc(T.v, &rcount, R)) || (e = sam_alloc(T.v, &rfirst, R)))
    return e;
  JOB_TRY(launch(tagk::tag_value_runs, gm, tagk::kThreads, s, V.text, ck2, ci2, va, vlen, head, rid, m, rpos, rlen));
  if ((e = sam_scan(rlen, nr, toff, part, s)) != BQSR_OK) return e;  // (nr <= m <= n: part is large enough)
  uint64_t tb64 = 0;
  HIP_TRY(hipMemcpyAsync(&tb64, toff + nr, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  uint8_t* d_text;
  if ((e = sam_alloc(T.v, &d_text, (size_t)tb64)) != BQSR_OK) return e;
  JOB_TRY(launch(tagk::tag_value_text, sam_grid(nr, tagk::kThreads, ctx->n_cu * 8), tagk::kThreads, s, V.text, ck2, ci2,
                 va, vlen, rpos, toff, nr, m, V.C.base, rtype, rcount, rfirst, d_text));
  TagRuns& G = g_tag_runs;
  const size_t r0 = G.type.size(), t0 = G.text.size();
  std::vector<uint64_t> ho(R + 1);
  G.type.resize(r0 + R);
  G.count.resize(r0 + R);
  G.first.resize(r0 + R);
  G.text.resize(t0 + (size_t)tb64);
  HIP_TRY(hipMemcpyAsync(G.type.data() + r0, rtype, R, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(G.count.data() + r0, rcount, R * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(G.first.data() + r0, rfirst, R * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(ho.data(), toff, (R + 1) * 8, hipMemcpyDeviceToHost, s));
  if (tb64) HIP_TRY(hipMemcpyAsync(G.text.data() + t0, d_text, (size_t)tb64, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (size_t r = 1; r <= R; ++r) G.toff.push_back((int64_t)(t0 + ho[r]));
  return BQSR_OK;
}

bool tag_arg_ok(const char* tag, int32_t hash_bits) { return tag && hash_bits >= 1 && hash_bits <= 64; }

void tag_sizes(bqsr_tag_value_sizes* out) {
  out->n_runs = (int64_t)g_tag_runs.type.size();
  out->text_bytes = (int64_t)g_tag_runs.text.size();
}

}  // namespace

extern "C" {

bqsr_status bqsr_sam_tag_counts(bqsr_context* ctx, const bqsr_sam* sm, void* stream, bqsr_tag_counts* out) {
  if (!ctx || !sm || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_tag_counts: bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  memset(out, 0, sizeof *out);
  g_tags_ms[TAGS_SCAN] = 0.0;
  const int64_t n = sm->n_reads;
  if (n == 0) return ok();
  SortTmp T;
  TagClock clock;
  unsigned long long* d;
  bqsr_status e;
  if ((e = tags_block(T, &d, s)) != BQSR_OK) return e;
  HIP_TRY(clock.mark(0, s));
  JOB_TRY(launch(tagk::tags_scan_sam, tags_grid(ctx, n), tagk::kThreads, s, sm->d_text, sm->line_span, sm->qual_span,
                 sm->raw_flag, n, d));
  HIP_TRY(clock.mark(1, s));
  return tags_finish(d, s, clock, out);
}

bqsr_status bqsr_arrow_tag_counts(bqsr_context* ctx, const bqsr_tags_chunk* chunks, int32_t n_chunks, void* stream,
                                  bqsr_tag_counts* out) {
  if (!ctx || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_tag_counts: bad arguments");
  bqsr_status e;
  if ((e = tags_chunks_ok(chunks, n_chunks, "bqsr_arrow_tag_counts")) != BQSR_OK) return e;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  memset(out, 0, sizeof *out);
  g_tags_ms[TAGS_SCAN] = 0.0;
  SortTmp T;
  TagClock clock;
  unsigned long long* d;
  if ((e = tags_block(T, &d, s)) != BQSR_OK) return e;
  double ms = 0.0;
  int64_t base = 0;
  for (int32_t c = 0; c < n_chunks; ++c) {
    const int64_t m = chunks[c].n_reads;
    if (m == 0) continue;
    SortTmp stage;
    tagk::ArrowTags C;
    if ((e = tags_stage(stage, chunks[c], base, s, &C)) != BQSR_OK) return e;
    HIP_TRY(clock.mark(0, s));
    JOB_TRY(launch(tagk::tags_scan_arrow, tags_grid(ctx, m), tagk::kThreads, s, C, d));
    HIP_TRY(clock.mark(1, s));
    HIP_TRY(hipStreamSynchronize(s));  // (the staging goes)
    clock.add(ms, 0, 1);
    base += m;
  }
  HIP_TRY(clock.mark(0, s));
  HIP_TRY(clock.mark(1, s));
  e = tags_finish(d, s, clock, out);
  g_tags_ms[TAGS_SCAN] = ms;  // the chunks' sum, without the empty span tags_finish read
  return e;
}

bqsr_status bqsr_sam_tag_values(bqsr_context* ctx, const bqsr_sam* sm, const char* tag, int32_t hash_bits,
                                void* stream, bqsr_tag_value_sizes* out) {
  if (!ctx || !sm || !out || !tag_arg_ok(tag, hash_bits))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_tag_values: bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  g_tag_runs.clear();
  g_tags_ms[TAGS_VALUES] = 0.0;
  tag_sizes(out);
  tagk::Values V{};
  V.text = sm->d_text;
  V.line_span = sm->line_span;
  V.qual_span = sm->qual_span;
  V.raw_flag = sm->raw_flag;
  V.n = sm->n_reads;
  V.tag = (uint32_t)(uint8_t)tag[0] | ((uint32_t)(uint8_t)tag[1] << 8);
  V.bits = hash_bits;
  if (V.n == 0) return ok();
  TagClock clock;
  HIP_TRY(clock.mark(0, s));
  const bqsr_status e = tag_values_run(ctx, V, s);
  if (e != BQSR_OK) {
    g_tag_runs.clear();
    return e;
  }
  HIP_TRY(clock.mark(1, s));
  HIP_TRY(hipStreamSynchronize(s));
  clock.add(g_tags_ms[TAGS_VALUES], 0, 1);
  tag_sizes(out);
  return ok();
}

bqsr_status bqsr_arrow_tag_values(bqsr_context* ctx, const bqsr_tags_chunk* chunks, int32_t n_chunks, const char* tag,
                                  int32_t hash_bits, void* stream, bqsr_tag_value_sizes* out) {
  if (!ctx || !out || !tag_arg_ok(tag, hash_bits))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_tag_values: bad arguments");
  bqsr_status e;
  if ((e = tags_chunks_ok(chunks, n_chunks, "bqsr_arrow_tag_values")) != BQSR_OK) return e;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  g_tag_runs.clear();
  g_tags_ms[TAGS_VALUES] = 0.0;
  tag_sizes(out);
  TagClock clock;
  double ms = 0.0;
  int64_t base = 0;
  for (int32_t c = 0; c < n_chunks; ++c) {
    const int64_t m = chunks[c].n_reads;
    if (m == 0) continue;
    SortTmp stage;
    tagk::Values V{};
    if ((e = tags_stage(stage, chunks[c], base, s, &V.C)) != BQSR_OK) {
      g_tag_runs.clear();
      return e;
    }
    V.text = V.C.bytes;
    V.n = m;
    V.tag = (uint32_t)(uint8_t)tag[0] | ((uint32_t)(uint8_t)tag[1] << 8);
    V.bits = hash_bits;
    HIP_TRY(clock.mark(0, s));
    if ((e = tag_values_run(ctx, V, s)) != BQSR_OK) {
      g_tag_runs.clear();
      return e;
    }
    HIP_TRY(clock.mark(1, s));
    HIP_TRY(hipStreamSynchronize(s));
    clock.add(ms, 0, 1);
    base += m;
  }
  g_tags_ms[TAGS_VALUES] = ms;
  tag_sizes(out);
  return ok();
}

bqsr_status bqsr_tag_values_fetch(const bqsr_tag_value_host* dst) {
  if (!dst) return fail(BQSR_ERR_INVALID_ARG, "bqsr_tag_values_fetch: null");
  const TagRuns& G = g_tag_runs;
  const size_t R = G.type.size();
  if ((R && (!dst->type || !dst->count || !dst->first_read)) || !dst->text_offsets || (!G.text.empty() && !dst->text))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_tag_values_fetch: null column");
  if (R) {
    memcpy(dst->type, G.type.data(), R);
    memcpy(dst->count, G.count.data(), R * 8);
    memcpy(dst->first_read, G.first.data(), R * 8);
  }
  memcpy(dst->text_offsets, G.toff.data(), (R + 1) * 8);
  if (!G.text.empty()) memcpy(dst->text, G.text.data(), G.text.size());
  return ok();
}

/* measurement only (tools/bench_adam.py --print-tags): the device-event times
 * of this thread's last counts call (its scan kernels) and last values call
 * (the value kernels with their sorts and scans) */
bqsr_status bqsr_tags_kernel_times(double* scan_ms, double* values_ms) {
  if (scan_ms) *scan_ms = g_tags_ms[TAGS_SCAN];
  if (values_ms) *values_ms = g_tags_ms[TAGS_VALUES];
  return BQSR_OK;
}

}  // extern "C"
