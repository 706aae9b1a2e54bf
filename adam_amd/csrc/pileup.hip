// `adam reads2ref` on the device (include/adam_sam.h: bqsr_sam_pileup_*,
// bqsr_arrow_pileup_*): Reads2PileupProcessor.readToPileups
// (core/rdd/Reads2PileupProcessor.scala:34-197) over MdTag
// (core/util/MdTag.scala:38-98, 247-269) and RichADAMRecord's qualityScores /
// end (core/rich/RichADAMRecord.scala:43, 77-87): every read becomes one
// ADAMPileup row per M, I, D or S base of its CIGAR.
//
// Two passes over reads [r0, r0 + n) of a parse layout (a SAM / BAM parse, or
// the layout bqsr_arrow_load builds from ADAMRecord Parquet), one core for
// both front ends:
//
//   pileup_count  a lane per read.  The full walk of readToPileups without
//       its output: the MD tag is parsed (MdTag.apply's grammar, as md_scan)
//       into the read's sparse list of non-match reference offsets -- u32
//       entries offset << 6 | delete << 5 | Base index, ascending, kept in
//       scratch at the read's md_off -- then the CIGAR is walked against that
//       list, the sequence and the quals in the order the reference evaluates
//       them, so that the first exception it would raise decides the read's
//       status.  The lowest throwing read index, with its status, is kept by
//       atomicMin.  The pass leaves per CIGAR element the rows, read bases and
//       reference offset before it (the prefixes pass 2 searches), and per
//       read its row count, readEnd and mapq.
//   (scan)        exclusive scan of the row counts: every read's first row.
//   pileup_emit   a lane per OUTPUT ROW: a wavefront takes aligned groups of 64
//       consecutive rows, so every column store is one contiguous 64-, 256- or
//       512-byte wave store and every validity word is one ballot stored by
//       lane 0.  A lane finds its read by binary search over the row prefix
//       (first narrowed, by searches every lane does alike, to the reads the
//       group touches; a wavefront's groups are consecutive, so only its
//       first group searches the whole prefix and the later ones gallop on
//       from where the last ended), its position in the walk as count - 1 - k (the
//       reference builds a read's list by prepending: rows come out in
//       reverse walk order), its CIGAR element by binary search over the
//       element prefix and its MD entry by binary search over the read's
//       list: no per-row work is linear in the CIGAR or the MD.
//
// Included by bqsr_capi.cpp after arrow_ingest.hip.

#include "adam_fields.h"

namespace pilk {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kMaxMdOffset = (1u << 26) - 1;  // the offset field of an MD entry
constexpr int64_t kMaxReadRows = 2147483647LL;     // rows and read bases of one read (u32 prefixes)

// index in adam.avdl's Base enum (A C T G U N X K M R Y S W B V H D), -1: no
// symbol (Base.valueOf throws).  Case-sensitive, as valueOf is.
__device__ __forceinline__ int base_index(uint8_t c) {
  switch (c) {
    case 'A': return 0;
    case 'C': return 1;
    case 'T': return 2;
    case 'G': return 3;
    case 'U': return 4;
    case 'N': return 5;
    case 'X': return 6;
    case 'K': return 7;
    case 'M': return 8;
    case 'R': return 9;
    case 'Y': return 10;
    case 'S': return 11;
    case 'W': return 12;
    case 'B': return 13;
    case 'V': return 14;
    case 'H': return 15;
    case 'D': return 16;
    default: return -1;
  }
}

// the parse layout (bqsr_sam / bqsr_arrow columns)
struct Reads {
  const uint32_t* flags;
  const int64_t* start;
  const uint64_t *seq_off, *qual_off, *cig_off, *md_off;
  const uint8_t *seq, *qual, *md;
  const uint32_t* cig;
  // mapq: from each read's line (a SAM / BAM parse) ...
  const uint8_t* text;
  const uint64_t* line_span;
  const int32_t* sq_id;
  // ... or given per read (Arrow; in_mapq_ok null: every mapq null)
  const int32_t* in_mapq;
  const uint8_t* in_mapq_ok;
};

struct Scratch {
  // per CIGAR element of the parse (at the read's cig_off): what lies before it
  uint32_t* rowpre;   // rows
  uint32_t* readpre;  // read bases
  int64_t* refpre;    // reference offset from start
  uint32_t* mdent;    // per MD byte of the parse (at the read's md_off): the read's entries
  // per read of the range
  uint64_t* cnt;      // rows
  uint32_t* md_n;     // entries
  int64_t* rend;      // readEnd
  int32_t* mapq;
  uint8_t* mapq_ok;
};

// MdTag.apply: entries of the non-match positions; 0, BQSR_ERR_MD_PARSE or
// BQSR_ERR_UNSUPPORTED (an entry beyond kMaxMdOffset)
__device__ int md_entries(const uint8_t* md, int64_t n, uint32_t* ent, uint32_t* n_ent, int64_t* span) {
  int64_t off = 0, pos = 0;
  uint32_t ne = 0;
  *n_ent = 0;
  *span = 0;
  if (n == 0) return 0;
  auto digits = [&]() -> bool {
    const int64_t b = off;
    int64_t v = 0;
    while (off < n && md[off] >= '0' && md[off] <= '9') {
      v = v * 10 + (md[off] - '0');
      if (v > 2147483647LL) return false;  // toInt overflow
      ++off;
    }
    if (off == b) return false;
    pos += v;
    return true;
  };
  if (!digits()) return BQSR_ERR_MD_PARSE;
  bool far = false;
  while (off < n) {
    uint32_t del = 0;
    if (md[off] == '^') {
      ++off;
      del = 1;
    }
    const int64_t b = off;
    while (off < n && bqsr::md_base(md[off])) {
      uint8_t c = md[off];
      if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);  // toUpperCase
      if (pos > (int64_t)kMaxMdOffset) far = true;
      else ent[ne++] = ((uint32_t)pos << 6) | (del << 5) | (uint32_t)base_index(c);
      ++pos;
      ++off;
    }
    if (off == b) return BQSR_ERR_MD_PARSE;
    if (!digits()) return BQSR_ERR_MD_PARSE;
  }
  if (far) return BQSR_ERR_UNSUPPORTED;
  *n_ent = ne;
  *span = pos;
  return 0;
}

struct CountParams {
  Reads R;
  Scratch X;
  int64_t r0, n;
  unsigned long long* err;  // atomicMin of (read index in the range) << 8 | status
};

// readToPileups for read r without its output: the status of the first
// exception in the reference's evaluation order, the row count otherwise
__device__ int walk_read(const CountParams& P, int64_t i, int64_t r, uint64_t* rows_out) {
  const Reads& R = P.R;
  const uint32_t f = R.flags[r];
  *rows_out = 0;
  P.X.md_n[i] = 0;
  P.X.rend[i] = 0;
  // a null cigar or mismatchingPositions: no pileups
  if (!(f & BQSR_F_HAS_CIGAR) || !(f & BQSR_F_HAS_MD)) return 0;
  if (!(f & BQSR_F_HAS_START)) return BQSR_ERR_NULL_FIELD;  // MdTag(md, start): start unboxed
  const uint64_t m0 = R.md_off[r];
  uint32_t* ent = P.X.mdent + m0;
  uint32_t n_ent;
  int64_t span;
  const int st = md_entries(R.md + m0, (int64_t)(R.md_off[r + 1] - m0), ent, &n_ent, &span);
  if (st) return st;
  P.X.md_n[i] = n_ent;
  const uint64_t c0 = R.cig_off[r];
  const int64_t ne = (int64_t)(R.cig_off[r + 1] - c0);
  const bool has_seq = f & BQSR_F_HAS_SEQ, has_qual = f & BQSR_F_HAS_QUAL, mapped = f & BQSR_F_MAPPED;
  const uint64_t s0 = R.seq_off[r], q0 = R.qual_off[r];
  const int64_t ls = has_seq ? (int64_t)(R.seq_off[r + 1] - s0) : 0;
  const int64_t lq = has_qual ? (int64_t)(R.qual_off[r + 1] - q0) : 0;
  int64_t rows = 0, rp = 0, ro = 0;  // rows so far, readPos, referencePos - start
  uint32_t j = 0;                    // first entry at or after ro
  // baseFromSequence(rp)
  auto seq_base = [&]() -> int {
    if (!has_seq) return BQSR_ERR_NULL_FIELD;
    if (rp >= ls || base_index(R.seq[s0 + rp]) < 0) return BQSR_ERR_PILEUP;
    return 0;
  };
  // populatePileupFromReference: record.end (None when unmapped), qualityScores(rp)
  auto populate = [&]() -> int {
    if (!mapped) return BQSR_ERR_PILEUP;
    if (!has_qual) return BQSR_ERR_NULL_FIELD;
    if (rp >= lq) return BQSR_ERR_PILEUP;
    return 0;
  };
  for (int64_t k = 0; k < ne; ++k) {
    const uint32_t e = R.cig[c0 + k], op = bqsr::cig_op(e);
    const int64_t len = bqsr::cig_len(e);
    if (rows > kMaxReadRows || rp > kMaxReadRows) return BQSR_ERR_UNSUPPORTED;
    P.X.rowpre[c0 + k] = (uint32_t)rows;
    P.X.readpre[c0 + k] = (uint32_t)rp;
    P.X.refpre[c0 + k] = ro;
    int s;
    if (op == BQSR_CIGAR_M) {
      for (int64_t b = 0; b < len; ++b) {
        while (j < n_ent && (int64_t)(ent[j] >> 6) < ro) ++j;
        const bool hit = j < n_ent && (int64_t)(ent[j] >> 6) == ro;
        if (!hit && ro < span) {  // isMatch: the reference base is the read's
          if ((s = seq_base())) return s;
        } else if (!hit || (ent[j] & 32u)) {
          return BQSR_ERR_PILEUP;  // neither match nor mismatch: a delete there, or the MD has ended
        }
        if ((s = populate()) || (s = seq_base())) return s;
        ++rp;
        ++ro;
      }
      rows += len;
    } else if (op == BQSR_CIGAR_I) {
      if (!has_seq) return BQSR_ERR_NULL_FIELD;  // getSequence.toString.substring(rp, rp + len)
      if (rp + len > ls) return BQSR_ERR_PILEUP;
      for (int64_t b = 0; b < len; ++b) {
        if (base_index(R.seq[s0 + rp]) < 0) return BQSR_ERR_PILEUP;
        if ((s = populate())) return s;
        ++rp;
      }
      rows += len;
    } else if (op == BQSR_CIGAR_D) {
      for (int64_t b = 0; b < len; ++b) {
        while (j < n_ent && (int64_t)(ent[j] >> 6) < ro) ++j;
        if (!(j < n_ent && (int64_t)(ent[j] >> 6) == ro && (ent[j] & 32u))) return BQSR_ERR_PILEUP;
        if ((s = populate())) return s;  // the quality at the NEXT read base
        ++ro;
      }
      rows += len;
    } else if (op == BQSR_CIGAR_S) {
      for (int64_t b = 0; b < len; ++b) {
        if ((s = seq_base()) || (s = populate())) return s;
        ++rp;
      }
      rows += len;
    } else {
      if (op == BQSR_CIGAR_EQ || op == BQSR_CIGAR_X) rp += len;
      if (bqsr::consumes_ref(op)) ro += len;
    }
  }
  if (rows > kMaxReadRows || rp > kMaxReadRows) return BQSR_ERR_UNSUPPORTED;
  // RichADAMRecord.end: start + the lengths of the reference-consuming elements
  P.X.rend[i] = R.start[r] + ro;
  *rows_out = (uint64_t)rows;
  return 0;
}

// mapq of read r (SAMRecordConverter.scala:46-54: only with a reference, and
// not 255; Arrow: the column's entry); false: null
__device__ __forceinline__ bool read_mapq(const Reads& R, int64_t r, int32_t* out) {
  int32_t q = 0;
  bool has = false;
  if (R.text) {
    const int64_t e = (int64_t)R.line_span[2 * r + 1];
    int64_t p = (int64_t)R.line_span[2 * r], a4 = 0, b4 = 0;
    for (int k = 0; k < 5; ++k) {  // MAPQ is field 5 of the line (the parse saw 11 fields)
      const int64_t fa = p;
      while (p < e && R.text[p] != '\t') ++p;
      if (k == 4) a4 = fa, b4 = p;
      if (p < e) ++p;
    }
    int64_t v;
    has = adamk::mapq_field(R.text, a4, b4, R.sq_id[r], &v);
    q = has ? (int32_t)v : 0;
  } else if (R.in_mapq_ok && R.in_mapq_ok[r]) {
    has = true;
    q = R.in_mapq[r];
  }
  *out = q;
  return has;
}

extern "C" __global__ void __launch_bounds__(kThreads) pileup_count(CountParams P) {
  const Reads& R = P.R;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = P.r0 + i;
    uint64_t rows;
    const int st = walk_read(P, i, r, &rows);
    P.X.cnt[i] = st ? 0 : rows;
    if (st) atomicMin(P.err, ((unsigned long long)i << 8) | (unsigned long long)st);
    int32_t q;
    const bool has = read_mapq(R, r, &q);
    P.X.mapq[i] = q;
    P.X.mapq_ok[i] = has;
  }
}

// Arrow's mapq column of one chunk into the per-read form (base = the
// chunk's first read)
extern "C" __global__ void __launch_bounds__(kThreads) pileup_mapq_chunk(const int32_t* v, const uint8_t* valid,
                                                                         int64_t n, int32_t* out, uint8_t* out_ok) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const bool ok = !valid || ((valid[r >> 3] >> (r & 7)) & 1u);
    out[r] = ok ? v[r] : 0;
    out_ok[r] = ok;
  }
}

struct Cols {
  int32_t* read;
  int64_t* position;
  int32_t *range_offset, *range_length;
  uint8_t *reference_base, *read_base;
  int32_t *sanger, *mapq, *soft, *rev;
  int64_t *read_start, *read_end;
  uint64_t *v_range, *v_reference_base, *v_read_base, *v_mapq;  // [ceil(n_rows / 64)]
};

struct EmitParams {
  Reads R;
  Scratch X;
  const uint64_t* rs;  // [n + 1] first row of each read of the range
  int64_t r0, n, n_rows;
  Cols C;
};

// the largest i in [a, b] with rs[i] <= g (rs[a] <= g)
__device__ __forceinline__ int64_t last_le(const uint64_t* rs, int64_t a, int64_t b, uint64_t g) {
  while (a < b) {
    const int64_t m = (a + b + 1) >> 1;
    if (rs[m] <= g) a = m;
    else b = m - 1;
  }
  return a;
}

// the same from a known a with rs[a] <= g, in steps 1, 2, 4, ..: a few loads when the answer is near
__device__ __forceinline__ int64_t gallop(const uint64_t* rs, int64_t n, int64_t a, uint64_t g) {
  int64_t step = 1;
  while (a + step <= n - 1 && rs[a + step] <= g) {
    a += step;
    step <<= 1;
  }
  return last_le(rs, a, min(a + step - 1, n - 1), g);
}

extern "C" __global__ void __launch_bounds__(kThreads) pileup_emit(EmitParams P) {
  const Reads& R = P.R;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t groups = (P.n_rows + 63) >> 6;
  // a wavefront takes a run of consecutive groups: the first group's read by
  // a search over the whole prefix, every later one by galloping on from the
  // read the group before it ended in (a chain of ~40 dependent loads per
  // group, when every group searched from scratch, was what bounded the kernel)
  const int64_t per = (groups + waves - 1) / waves;
  const int64_t grp_end = min(groups, (wave0 + 1) * per);
  int64_t hi = -1;
  for (int64_t grp = wave0 * per; grp < grp_end; ++grp) {
    const int64_t g0 = grp << 6;
    const int64_t g = g0 + lane;
    const bool live = g < P.n_rows;
    const uint64_t gl = (uint64_t)(live ? g : P.n_rows - 1);  // (idle lanes follow the last row, store nothing)
    // the reads this group's rows belong to (the same searches in every lane), then this row's
    const int64_t lo = hi < 0 ? last_le(P.rs, 0, P.n - 1, (uint64_t)g0) : gallop(P.rs, P.n, hi, (uint64_t)g0);
    hi = gallop(P.rs, P.n, lo, (uint64_t)min(g0 + 63, P.n_rows - 1));
    const int64_t i = last_le(P.rs, lo, hi, gl);
    const int64_t r = P.r0 + i;
    const uint64_t first = P.rs[i];
    const uint64_t count = P.rs[i + 1] - first;
    const uint32_t w = (uint32_t)(count - 1 - (gl - first));  // position in the walk: rows are prepended
    // the CIGAR element holding walk position w
    const uint64_t c0 = R.cig_off[r];
    int64_t ea = 0, eb = (int64_t)(R.cig_off[r + 1] - c0) - 1;
    while (ea < eb) {
      const int64_t m = (ea + eb + 1) >> 1;
      if (P.X.rowpre[c0 + m] <= w) ea = m;
      else eb = m - 1;
    }
    const uint32_t e = R.cig[c0 + ea], op = bqsr::cig_op(e);
    const uint32_t k = w - P.X.rowpre[c0 + ea];  // index within the element
    const bool is_m = op == BQSR_CIGAR_M, is_d = op == BQSR_CIGAR_D;
    const int64_t rp = (int64_t)P.X.readpre[c0 + ea] + (is_d ? 0 : k);
    const int64_t ro = P.X.refpre[c0 + ea] + ((is_m || is_d) ? k : 0);
    const uint32_t f = R.flags[r];
    const int64_t start = R.start[r];
    // the MD entry at ro (M: a mismatch, D: the deleted base)
    int ref_base = -1;
    if (is_m || is_d) {
      const uint32_t* ent = P.X.mdent + R.md_off[r];
      int64_t a = 0, b = P.X.md_n[i];
      while (a < b) {  // first entry with offset >= ro
        const int64_t m = (a + b) >> 1;
        if ((int64_t)(ent[m] >> 6) < ro) a = m + 1;
        else b = m;
      }
      if (a < (int64_t)P.X.md_n[i] && (int64_t)(ent[a] >> 6) == ro) ref_base = (int)(ent[a] & 31u);
    }
    int read_base = -1;
    if (!is_d) {
      read_base = base_index(R.seq[R.seq_off[r] + rp]);
      if (is_m && ref_base < 0) ref_base = read_base;  // a match
    }
    const int32_t sanger = (int32_t)(int8_t)(uint8_t)(R.qual[R.qual_off[r] + rp] - 33);
    const bool ranged = !is_m;
    const bool has_mapq = P.X.mapq_ok[i];
    const uint64_t vr = __builtin_amdgcn_ballot_w64(live && ranged);
    const uint64_t vb = __builtin_amdgcn_ballot_w64(live && ref_base >= 0);
    const uint64_t vd = __builtin_amdgcn_ballot_w64(live && read_base >= 0);
    const uint64_t vq = __builtin_amdgcn_ballot_w64(live && has_mapq);
    if (lane == 0) {
      P.C.v_range[grp] = vr;
      P.C.v_reference_base[grp] = vb;
      P.C.v_read_base[grp] = vd;
      P.C.v_mapq[grp] = vq;
    }
    if (live) {
      P.C.read[g] = (int32_t)i;
      P.C.position[g] = start + ro;
      P.C.range_offset[g] = ranged ? (int32_t)k : 0;
      P.C.range_length[g] = ranged ? (int32_t)bqsr::cig_len(e) : 0;
      P.C.reference_base[g] = (uint8_t)(ref_base >= 0 ? ref_base : 0);
      P.C.read_base[g] = (uint8_t)(read_base >= 0 ? read_base : 0);
      P.C.sanger[g] = sanger;
      P.C.mapq[g] = has_mapq ? P.X.mapq[i] : 0;
      P.C.soft[g] = op == BQSR_CIGAR_S ? 1 : 0;
      P.C.rev[g] = (f & BQSR_F_NEG_STRAND) ? 1 : 0;
      P.C.read_start[g] = start;
      P.C.read_end[g] = P.X.rend[i];
    }
  }
}

}  // namespace pilk

namespace {

// the scratch and the columns of one parse handle, kept across calls
struct PileupState {
  pilk::Scratch X{};
  int64_t cap_cig = -1, cap_md = -1, cap_n = -1, cap_rows = -1;
  uint64_t *rs = nullptr, *part = nullptr;
  unsigned long long* err = nullptr;
  // bqsr_arrow_pileup_prepare: the mapq column, per read of the handle
  int32_t* a_mapq = nullptr;
  uint8_t* a_mapq_ok = nullptr;
  bool a_loaded = false;
  pilk::Cols C{};
  uint8_t* col_block = nullptr;
  int64_t r0 = 0, n = 0, n_rows = 0;
  bool prepared = false;
  StageClock<4> clock;
  std::vector<void*> per_parse, per_range;
  static void drop(std::vector<void*>& v) {
    for (void* p : v) (void)hipFree(p);
    v.clear();
  }
  ~PileupState() {
    drop(per_parse);
    drop(per_range);
    for (void* p : {(void*)err, (void*)a_mapq, (void*)a_mapq_ok, (void*)col_block})
      if (p) (void)hipFree(p);
  }
};

// the two kernels' times of the calling thread's last prepare / columns, and the clock's marks around them
enum { PILEUP_COUNT, PILEUP_EMIT, PILEUP_STAGES };
enum { PILEUP_COUNT_0, PILEUP_COUNT_1, PILEUP_EMIT_0, PILEUP_EMIT_1 };
thread_local double g_pileup_ms[PILEUP_STAGES] = {0.0, 0.0};

struct PileupView {
  pilk::Reads R;
  int64_t n_reads, cig_ops, md_bytes;
};

unsigned pileup_grid(const bqsr_context* ctx, int64_t blocks) {
  const int64_t cap = ctx->tune_pileup_grid > 0 ? ctx->tune_pileup_grid : (int64_t)ctx->n_cu * 8;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, cap));
}

const char* pileup_what(int status) {
  switch (status) {
    case BQSR_ERR_NULL_FIELD:
      return "a null start, sequence or qual (the reference throws a NullPointerException)";
    case BQSR_ERR_MD_PARSE:
      return "an MD tag MdTag.apply rejects";
    case BQSR_ERR_PILEUP:
      return "an exception inside readToPileups (a base outside the Base enum, sequence or quals shorter than the "
             "CIGAR, CIGAR and MD disagreeing, or pileups of a read that is not mapped)";
    default:
      return "beyond the device path's limits (a mismatch or deleted base 2^26 or more positions after the read's "
             "start, or 2^31 or more rows or read bases in one read)";
  }
}

bqsr_status pileup_prepare(bqsr_context* ctx, PileupState& A, const PileupView& V, int64_t r0, int64_t n,
                           hipStream_t s, bqsr_pileup_sizes* out, const char* who) {
  A.prepared = false;
  out->n_reads = n;
  out->n_rows = 0;
  out->bitmap_words = 0;
  bqsr_status e;
  if (!A.err) HIP_TRY(hipMalloc((void**)&A.err, 8));
  if (A.cap_cig < V.cig_ops || A.cap_md < V.md_bytes) {
    PileupState::drop(A.per_parse);
    A.cap_cig = A.cap_md = -1;
    const size_t nc = (size_t)V.cig_ops, nm = (size_t)V.md_bytes;
    if ((e = sam_alloc(A.per_parse, &A.X.rowpre, nc)) || (e = sam_alloc(A.per_parse, &A.X.readpre, nc)) ||
        (e = sam_alloc(A.per_parse, &A.X.refpre, nc)) || (e = sam_alloc(A.per_parse, &A.X.mdent, nm)))
      return e;
    A.cap_cig = V.cig_ops;
    A.cap_md = V.md_bytes;
  }
  if (A.cap_n < n) {
    PileupState::drop(A.per_range);
    A.cap_n = -1;
    const size_t N = (size_t)n + 1;
    if ((e = sam_alloc(A.per_range, &A.X.cnt, N)) || (e = sam_alloc(A.per_range, &A.rs, N)) ||
        (e = sam_alloc(A.per_range, &A.part, N / samk::kScanChunk + 2)) || (e = sam_alloc(A.per_range, &A.X.md_n, N)) ||
        (e = sam_alloc(A.per_range, &A.X.rend, N)) || (e = sam_alloc(A.per_range, &A.X.mapq, N)) ||
        (e = sam_alloc(A.per_range, &A.X.mapq_ok, N)))
      return e;
    A.cap_n = n;
  }
  A.r0 = r0;
  A.n = n;
  A.n_rows = 0;
  g_pileup_ms[PILEUP_COUNT] = g_pileup_ms[PILEUP_EMIT] = 0.0;
  if (n == 0) {
    A.prepared = true;
    return ok();
  }
  HIP_TRY(hipMemsetAsync(A.err, 0xFF, 8, s));
  pilk::CountParams P{V.R, A.X, r0, n, A.err};
  HIP_TRY(A.clock.mark(PILEUP_COUNT_0, s));
  JOB_TRY(launch(pilk::pileup_count, pileup_grid(ctx, (n + pilk::kThreads - 1) / pilk::kThreads), pilk::kThreads, s,
                 P));
  HIP_TRY(A.clock.mark(PILEUP_COUNT_1, s));
  if ((e = sam_scan(A.X.cnt, n, A.rs, A.part, s)) != BQSR_OK) return e;
  unsigned long long ew = ~0ull;
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&ew, A.err, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&total, A.rs + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  A.clock.add(g_pileup_ms[PILEUP_COUNT], PILEUP_COUNT_0, PILEUP_COUNT_1);
  if (ew != ~0ull) {
    const int status = (int)(ew & 0xFF);
    const int64_t read = r0 + (int64_t)(ew >> 8);
    return fail((bqsr_status)status, std::string(who) + ": read " + std::to_string(read) + ": " + pileup_what(status),
                read);
  }
  if (total > (uint64_t)INT32_MAX)
    return fail(BQSR_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 - 1 pileups in one call (take fewer reads)");
  A.n_rows = (int64_t)total;
  out->n_rows = A.n_rows;
  out->bitmap_words = (A.n_rows + 63) / 64;
  A.prepared = true;
  return ok();
}

// the emit pass over the prepared range into the state's columns (queued on s; m = A.n_rows > 0)
bqsr_status pileup_emit_columns(bqsr_context* ctx, PileupState& A, const PileupView& V, hipStream_t s) {
  const int64_t m = A.n_rows;
  if (A.cap_rows < m) {  // one block, carved: the 8-byte columns first, every column 8-byte aligned
    if (A.col_block) (void)hipFree(A.col_block);
    A.col_block = nullptr;
    A.cap_rows = -1;
    const size_t M = ((size_t)m + 63) & ~(size_t)63;
    HIP_TRY(hipMalloc((void**)&A.col_block, M * (3 * 8 + 7 * 4 + 2) + 4 * (M / 64) * 8));
    A.cap_rows = (int64_t)M;
  }
  {
    const size_t M = (size_t)A.cap_rows;
    uint8_t* p = A.col_block;
    auto take = [&](auto** q, size_t count) {
      *q = (std::remove_reference_t<decltype(**q)>*)p;
      p += count * sizeof(**q);
    };
    take(&A.C.position, M);
    take(&A.C.read_start, M);
    take(&A.C.read_end, M);
    take(&A.C.v_range, M / 64);
    take(&A.C.v_reference_base, M / 64);
    take(&A.C.v_read_base, M / 64);
    take(&A.C.v_mapq, M / 64);
    take(&A.C.read, M);
    take(&A.C.range_offset, M);
    take(&A.C.range_length, M);
    take(&A.C.sanger, M);
    take(&A.C.mapq, M);
    take(&A.C.soft, M);
    take(&A.C.rev, M);
    take(&A.C.reference_base, M);
    take(&A.C.read_base, M);
  }
  pilk::EmitParams P{V.R, A.X, A.rs, A.r0, A.n, m, A.C};
  const int64_t groups = (m + 63) / 64;
  HIP_TRY(A.clock.mark(PILEUP_EMIT_0, s));
  JOB_TRY(launch(pilk::pileup_emit, pileup_grid(ctx, (groups + pilk::kWaves - 1) / pilk::kWaves), pilk::kThreads, s,
                 P));
  HIP_TRY(A.clock.mark(PILEUP_EMIT_1, s));
  return BQSR_OK;
}

bqsr_status pileup_columns(bqsr_context* ctx, PileupState& A, const PileupView& V, const bqsr_pileup_host* dst,
                           hipStream_t s, const char* who) {
  if (!A.prepared) return fail(BQSR_ERR_INVALID_ARG, std::string(who) + " before its prepare call");
  g_pileup_ms[PILEUP_EMIT] = 0.0;
  const int64_t m = A.n_rows;
  if (m == 0) return ok();
  const size_t W = (size_t)((m + 63) / 64);
  JOB_TRY(pileup_emit_columns(ctx, A, V, s));
  auto cp = [&](void* d, const void* src, size_t bytes) -> hipError_t {
    if (!d || !bytes) return hipSuccess;
    return hipMemcpyAsync(d, src, bytes, hipMemcpyDeviceToHost, s);
  };
  const size_t n = (size_t)m;
  hipError_t e = cp(dst->read, A.C.read, n * 4);
  if (e == hipSuccess) e = cp(dst->position, A.C.position, n * 8);
  if (e == hipSuccess) e = cp(dst->range_offset, A.C.range_offset, n * 4);
  if (e == hipSuccess) e = cp(dst->range_length, A.C.range_length, n * 4);
  if (e == hipSuccess) e = cp(dst->reference_base, A.C.reference_base, n);
  if (e == hipSuccess) e = cp(dst->read_base, A.C.read_base, n);
  if (e == hipSuccess) e = cp(dst->sanger_quality, A.C.sanger, n * 4);
  if (e == hipSuccess) e = cp(dst->map_quality, A.C.mapq, n * 4);
  if (e == hipSuccess) e = cp(dst->num_soft_clipped, A.C.soft, n * 4);
  if (e == hipSuccess) e = cp(dst->num_reverse_strand, A.C.rev, n * 4);
  if (e == hipSuccess) e = cp(dst->read_start, A.C.read_start, n * 8);
  if (e == hipSuccess) e = cp(dst->read_end, A.C.read_end, n * 8);
  if (e == hipSuccess) e = cp(dst->range_valid, A.C.v_range, W * 8);
  if (e == hipSuccess) e = cp(dst->reference_base_valid, A.C.v_reference_base, W * 8);
  if (e == hipSuccess) e = cp(dst->read_base_valid, A.C.v_read_base, W * 8);
  if (e == hipSuccess) e = cp(dst->map_quality_valid, A.C.v_mapq, W * 8);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(BQSR_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
  A.clock.add(g_pileup_ms[PILEUP_EMIT], PILEUP_EMIT_0, PILEUP_EMIT_1);
  return ok();
}

// the emit pass, the columns left on the device: *cols their device addresses
bqsr_status pileup_device_columns(bqsr_context* ctx, PileupState& A, const PileupView& V, bqsr_pileup_host* cols,
                                  hipStream_t s, const char* who) {
  if (!A.prepared) return fail(BQSR_ERR_INVALID_ARG, std::string(who) + " before its prepare call");
  g_pileup_ms[PILEUP_EMIT] = 0.0;
  *cols = bqsr_pileup_host{};
  if (A.n_rows == 0) return ok();
  JOB_TRY(pileup_emit_columns(ctx, A, V, s));
  HIP_TRY(hipStreamSynchronize(s));
  A.clock.add(g_pileup_ms[PILEUP_EMIT], PILEUP_EMIT_0, PILEUP_EMIT_1);
  const pilk::Cols& C = A.C;
  *cols = bqsr_pileup_host{C.read, C.position, C.range_offset, C.range_length, C.reference_base, C.read_base,
                           C.sanger, C.mapq, C.soft, C.rev, C.read_start, C.read_end, C.v_range,
                           C.v_reference_base, C.v_read_base, C.v_mapq};
  return ok();
}

// readStart and readEnd per read of the prepared range into host memory
bqsr_status pileup_read_spans(PileupState& A, const PileupView& V, int64_t* read_start, int64_t* read_end,
                              hipStream_t s, const char* who) {
  if (!A.prepared) return fail(BQSR_ERR_INVALID_ARG, std::string(who) + " before its prepare call");
  if (A.n == 0) return ok();
  const size_t bytes = (size_t)A.n * sizeof(int64_t);
  HIP_TRY(hipMemcpyAsync(read_start, V.R.start + A.r0, bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(read_end, A.X.rend, bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return ok();
}

PileupView pileup_view(const bqsr_sam* s) {
  PileupView V{};
  V.R = pilk::Reads{s->flags, s->start, s->seq_off, s->qual_off, s->cig_off, s->md_off, s->seq, s->qual, s->md, s->cig,
                    s->d_text, s->line_span, s->sq_id, nullptr, nullptr};
  V.n_reads = s->n_reads;
  V.cig_ops = s->cig_ops;
  V.md_bytes = s->md_bytes;
  return V;
}

PileupView pileup_view(const bqsr_arrow* a, const PileupState& A) {
  PileupView V{};
  V.R = pilk::Reads{a->flags, a->start, a->seq_off, a->qual_off, a->cig_off, a->md_off, a->seq, a->qual, a->md, a->cig,
                    nullptr, nullptr, nullptr, A.a_mapq, A.a_loaded ? A.a_mapq_ok : nullptr};
  V.n_reads = a->n;
  V.cig_ops = a->cig_ops;
  V.md_bytes = a->md_bytes;
  return V;
}

// the mapq column of an Arrow handle's reads (per chunk, host memory) onto the
// device, replacing an earlier one
bqsr_status pileup_arrow_mapq(bqsr_context* ctx, bqsr_arrow* a, PileupState& A, const int64_t* chunk_reads,
                              const int32_t* const* mapq, const uint8_t* const* mapq_validity, int32_t n_chunks,
                              hipStream_t s, const char* who) {
  int64_t tot = 0;
  for (int32_t c = 0; c < n_chunks; ++c) {
    if (chunk_reads[c] < 0) return fail(BQSR_ERR_INVALID_ARG, std::string(who) + ": negative chunk length");
    tot += chunk_reads[c];
  }
  if (tot != a->n) return fail(BQSR_ERR_INVALID_ARG, std::string(who) + ": the mapq chunks do not cover the reads");
  A.a_loaded = false;
  const size_t N = (size_t)std::max<int64_t>(a->n, 1);
  if (!A.a_mapq) HIP_TRY(hipMalloc((void**)&A.a_mapq, N * 4));
  if (!A.a_mapq_ok) HIP_TRY(hipMalloc((void**)&A.a_mapq_ok, N));
  HIP_TRY(hipMemsetAsync(A.a_mapq_ok, 0, N, s));
  SortTmp T;
  int64_t base = 0;
  bqsr_status e;
  for (int32_t c = 0; c < n_chunks; ++c) {
    const int64_t m = chunk_reads[c];
    if (m && mapq[c]) {  // (a NULL column: every mapq of the chunk null)
      HIP_TRY(hipMemcpyAsync(A.a_mapq + base, mapq[c], (size_t)m * 4, hipMemcpyHostToDevice, s));
      uint8_t* dv = nullptr;
      if (mapq_validity[c]) {
        if ((e = sam_alloc(T.v, &dv, (size_t)(m + 7) / 8)) != BQSR_OK) return e;
        HIP_TRY(hipMemcpyAsync(dv, mapq_validity[c], (size_t)(m + 7) / 8, hipMemcpyHostToDevice, s));
      }
      JOB_TRY(launch(pilk::pileup_mapq_chunk, sam_grid(m, pilk::kThreads, ctx->n_cu * 8), pilk::kThreads, s,
                     (const int32_t*)(A.a_mapq + base), dv, m, A.a_mapq + base, A.a_mapq_ok + base));
    }
    base += m;
  }
  HIP_TRY(hipStreamSynchronize(s));  // (the staging bitmaps are freed with T)
  A.a_loaded = true;
  return BQSR_OK;
}

}  // namespace

extern "C" {

bqsr_status bqsr_sam_pileup_prepare(bqsr_context* ctx, bqsr_sam* s, int64_t r0, int64_t n, void* stream,
                                    bqsr_pileup_sizes* out) {
  if (!ctx || !s || !out || r0 < 0 || n < 0 || r0 + n > s->n_reads)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_pileup_prepare: bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  return pileup_prepare(ctx, *job_state<PileupState>(s->pileup), pileup_view(s), r0, n, S(stream), out, "reads2ref");
}

bqsr_status bqsr_sam_pileup_columns(bqsr_context* ctx, bqsr_sam* s, const bqsr_pileup_host* dst, void* stream) {
  if (!ctx || !s || !dst) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_pileup_columns: bad arguments");
  if (!s->pileup) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_pileup_columns before bqsr_sam_pileup_prepare");
  HIP_TRY(hipSetDevice(ctx->device));
  return pileup_columns(ctx, *job_state<PileupState>(s->pileup), pileup_view(s), dst, S(stream),
                        "bqsr_sam_pileup_columns");
}

bqsr_status bqsr_arrow_pileup_prepare(bqsr_context* ctx, bqsr_arrow* a, int64_t r0, int64_t n,
                                      const int64_t* chunk_reads, const int32_t* const* mapq,
                                      const uint8_t* const* mapq_validity, int32_t n_chunks, void* stream,
                                      bqsr_pileup_sizes* out) {
  if (!ctx || !a || !out || r0 < 0 || n < 0 || r0 + n > a->n || n_chunks < 0 ||
      (n_chunks && (!chunk_reads || !mapq || !mapq_validity)))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_pileup_prepare: bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  PileupState& A = *job_state<PileupState>(a->pileup);
  if (n_chunks) {
    const bqsr_status e = pileup_arrow_mapq(ctx, a, A, chunk_reads, mapq, mapq_validity, n_chunks, s, "bqsr_arrow_pileup_prepare");
    if (e != BQSR_OK) return e;
  }
  return pileup_prepare(ctx, A, pileup_view(a, A), r0, n, s, out, "reads2ref");
}

bqsr_status bqsr_arrow_pileup_columns(bqsr_context* ctx, bqsr_arrow* a, const bqsr_pileup_host* dst, void* stream) {
  if (!ctx || !a || !dst) return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_pileup_columns: bad arguments");
  if (!a->pileup) return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_pileup_columns before bqsr_arrow_pileup_prepare");
  HIP_TRY(hipSetDevice(ctx->device));
  PileupState& A = *job_state<PileupState>(a->pileup);
  return pileup_columns(ctx, A, pileup_view(a, A), dst, S(stream), "bqsr_arrow_pileup_columns");
}

bqsr_status bqsr_sam_pileup_device_columns(bqsr_context* ctx, bqsr_sam* s, bqsr_pileup_host* cols, void* stream) {
  if (!ctx || !s || !cols) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_pileup_device_columns: bad arguments");
  if (!s->pileup) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_pileup_device_columns before bqsr_sam_pileup_prepare");
  HIP_TRY(hipSetDevice(ctx->device));
  return pileup_device_columns(ctx, *job_state<PileupState>(s->pileup), pileup_view(s), cols, S(stream),
                               "bqsr_sam_pileup_device_columns");
}

bqsr_status bqsr_arrow_pileup_device_columns(bqsr_context* ctx, bqsr_arrow* a, bqsr_pileup_host* cols, void* stream) {
  if (!ctx || !a || !cols) return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_pileup_device_columns: bad arguments");
  if (!a->pileup)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_pileup_device_columns before bqsr_arrow_pileup_prepare");
  HIP_TRY(hipSetDevice(ctx->device));
  PileupState& A = *job_state<PileupState>(a->pileup);
  return pileup_device_columns(ctx, A, pileup_view(a, A), cols, S(stream), "bqsr_arrow_pileup_device_columns");
}

bqsr_status bqsr_sam_pileup_read_spans(bqsr_context* ctx, bqsr_sam* s, int64_t* read_start, int64_t* read_end,
                                       void* stream) {
  if (!ctx || !s || !read_start || !read_end)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_pileup_read_spans: bad arguments");
  if (!s->pileup) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_pileup_read_spans before bqsr_sam_pileup_prepare");
  HIP_TRY(hipSetDevice(ctx->device));
  return pileup_read_spans(*job_state<PileupState>(s->pileup), pileup_view(s), read_start, read_end, S(stream),
                           "bqsr_sam_pileup_read_spans");
}

bqsr_status bqsr_arrow_pileup_read_spans(bqsr_context* ctx, bqsr_arrow* a, int64_t* read_start, int64_t* read_end,
                                         void* stream) {
  if (!ctx || !a || !read_start || !read_end)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_pileup_read_spans: bad arguments");
  if (!a->pileup) return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_pileup_read_spans before bqsr_arrow_pileup_prepare");
  HIP_TRY(hipSetDevice(ctx->device));
  PileupState& A = *job_state<PileupState>(a->pileup);
  return pileup_read_spans(A, pileup_view(a, A), read_start, read_end, S(stream), "bqsr_arrow_pileup_read_spans");
}

bqsr_status bqsr_pileup_kernel_times(double* count_ms, double* emit_ms) {
  if (count_ms) *count_ms = g_pileup_ms[PILEUP_COUNT];
  if (emit_ms) *emit_ms = g_pileup_ms[PILEUP_EMIT];
  return BQSR_OK;
}

}  // extern "C"
