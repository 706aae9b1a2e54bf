// `adam mpileup` on the device (include/adam_sam.h: bqsr_sam_mpileup_*,
// bqsr_arrow_mpileup_*): MpileupCommand.run (cli/MpileupCommand.scala:37-82)
// over PileupTraversable (core/util/PileupTraversable.scala:83-281) and MdTag
// (core/util/MdTag.scala:38-98, 247-269): the reads LocusPredicate keeps
// become match, mismatch, delete and insertion events, the events of one
// (reference run, position) become one line of text.
//
// One job over all reads of a parse layout (a SAM / BAM parse or the layout
// bqsr_arrow_load builds), which stays resident:
//
//   mp_keep, (scan), mp_compact   LocusPredicate per read; the kept reads'
//       indices in input order.
//   mp_walk       a lane per KEPT read.  readToPileups without its output:
//       the MD tag parsed by pileup.hip's md_entries, the CIGAR walked against
//       it in the order the reference evaluates things, so that the first
//       exception it would raise decides the read's status (the lowest
//       throwing read index is kept by atomicMin).  Leaves the event count,
//       per CIGAR element the events, read bases and reference offset before
//       it, the segment-start flag (referenceId differs from the kept read
//       before) and the order check (start below the kept read before, in
//       one segment: the lowest such read index by atomicMin).
//   (scans)       event counts -> first event of each read; segment flags ->
//       segment ids.
//   mp_emit       a lane per EVENT: its read by binary search over the event
//       prefix, its CIGAR element over the element prefix, its MD entry over
//       the read's list.  Key = segment | position | class over the bits in
//       use (match < mismatch < delete < insertion); payload = kept-read
//       index | the character to print | the reference-base code.
//   (sort)        stable rocprim::radix_sort_pairs over the key bits in use:
//       equal keys stay in read order, which is the reference's list order.
//   mp_heads      a line starts where (segment, position) changes; per event
//       its rendered length (1, 1, 3, 1 + digits(readLen) + readLen) and its
//       reference-base bit.
//   (scans, reduce_by_key)   line ids; event byte offsets; per line the OR of
//       the reference-base bits: one bit the base, none '?', several the
//       reference's AssertionError.
//   mp_first, mp_lines   first event of each line; per line numReads, the
//       header length, the line length; the lowest conflicting line by
//       atomicMin.  (scan) -> byte offset of every line.
//   mp_window     the largest run of whole lines from line0 within a byte
//       budget, by binary search over the line offsets.
//   mp_text       a lane per event of the window writes its one to three
//       bytes; the lane of a line's first event also writes the header, the
//       lane of its last the newline; insertion payloads ("+", the length,
//       the whole read sequence) are copied by the whole wavefront, one
//       insertion after the other.  Every byte's place follows from the
//       scans, none from the grid.
//
// Included by bqsr_capi.cpp after pileup.hip.

namespace mpk {

constexpr int kThreads = 256;
enum { kMatch = 0, kMismatch = 1, kDelete = 2, kInsert = 3 };
constexpr uint32_t kNoBase = 7;  // reference-base code of an insertion; 0..4 index kBaseChar
__device__ const char kBaseChar[5] = {'A', 'C', 'T', 'G', 'N'};

// code in PileupTraversable's Base enum (A C T G N) of an index in adam.avdl's
// (pilk::base_index); kNoBase: Base.withName throws
__device__ __forceinline__ uint32_t base5(int idx) {
  return idx >= 0 && idx <= 3 ? (uint32_t)idx : idx == 5 ? 4u : kNoBase;
}

struct BitOr {
  __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a | b; }
};

__device__ __forceinline__ int digits(uint64_t v) {
  int n = 1;
  while (v >= 10) {
    v /= 10;
    ++n;
  }
  return n;
}

// the nd decimal digits of v at out[o, o + nd)
__device__ __forceinline__ void put_dec(uint8_t* out, uint64_t o, uint64_t v, int nd) {
  for (int k = nd - 1; k >= 0; --k) {
    out[o + (uint64_t)k] = (uint8_t)('0' + v % 10);
    v /= 10;
  }
}

struct Reads {
  pilk::Reads R;
  const uint32_t* raw_flag;   // the SAM FLAG word (failedVendorQualityChecks), null: not known here
  const int32_t* ref_id;      // referenceId, -1: null
  const int32_t* ref_name;    // index into the name table, -1: null
  const uint8_t* name_valid;  // readName present, null: always
  int32_t n_names;            // entries of the name table
};

// LocusPredicate over the converted record (a FLAG-0 SAM record has every
// boolean false: quirk Q2)
extern "C" __global__ void __launch_bounds__(kThreads) mp_keep(Reads A, int64_t n, uint32_t* keep) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t f = A.R.flags[r];
    bool k = (f & BQSR_F_MAPPED) && (f & BQSR_F_PRIMARY) && !(f & BQSR_F_DUPLICATE);
    if (A.raw_flag && (A.raw_flag[r] & 0x200u)) k = false;
    keep[r] = k;
    if (r == 0) keep[n] = 0;
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) mp_compact(const uint32_t* keep, const uint32_t* kpos,
                                                                 int64_t n, int64_t* kidx) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
    if (keep[r]) kidx[kpos[r]] = r;
}

struct Scratch {
  // per CIGAR element of the parse (at the read's cig_off): what lies before it
  uint32_t* evpre;    // events
  uint32_t* readpre;  // read bases
  int64_t* refpre;    // reference offset from start
  uint32_t* mdent;    // per MD byte of the parse (at the read's md_off): the read's entries
  // per kept read
  uint64_t* cnt;      // events [nk + 1]
  uint32_t* md_n;     // entries
  uint32_t* segflag;  // 1: the read starts a segment
};

struct WalkParams {
  Reads A;
  Scratch X;
  const int64_t* kidx;
  int64_t nk;
  unsigned long long* err;       // atomicMin of (read index << 8 | status): what readToPileups / foreach throws
  unsigned long long* unsorted;  // atomicMin of the read index whose start decreases
  unsigned long long* maxpos;    // atomicMax of the last reference position an event may have
};

// readToPileups for read r without its output: the status of the first
// exception in the reference's evaluation order, the event count otherwise
__device__ int walk_read(const WalkParams& P, int64_t k, int64_t r, uint64_t* events_out, int64_t* ro_out) {
  const pilk::Reads& R = P.A.R;
  const uint32_t f = R.flags[r];
  *events_out = 0;
  *ro_out = 0;
  P.X.md_n[k] = 0;
  // a null cigar or mismatchingPositions: no events
  if (!(f & BQSR_F_HAS_CIGAR) || !(f & BQSR_F_HAS_MD)) return 0;
  const uint64_t m0 = R.md_off[r];
  uint32_t* ent = P.X.mdent + m0;
  uint32_t n_ent;
  int64_t span;
  const int st = pilk::md_entries(R.md + m0, (int64_t)(R.md_off[r + 1] - m0), ent, &n_ent, &span);
  if (st) return st;
  P.X.md_n[k] = n_ent;
  const uint64_t c0 = R.cig_off[r];
  const int64_t ne = (int64_t)(R.cig_off[r + 1] - c0);
  const bool has_seq = f & BQSR_F_HAS_SEQ;
  const uint64_t s0 = R.seq_off[r];
  const int64_t ls = has_seq ? (int64_t)(R.seq_off[r + 1] - s0) : 0;
  int32_t q;
  const bool no_name = P.A.name_valid && !P.A.name_valid[r];
  // mapq (.toInt), qual, referenceName: dereferenced by every event after the read name
  const bool no_rest = !pilk::read_mapq(R, r, &q) || !(f & BQSR_F_HAS_QUAL) || P.A.ref_name[r] < 0;
  int64_t events = 0, rp = 0, ro = 0;  // events so far, readPos, referencePos - start
  uint32_t j = 0;                      // first entry at or after ro
  for (int64_t e = 0; e < ne; ++e) {
    const uint32_t el = R.cig[c0 + e], op = bqsr::cig_op(el);
    const int64_t len = bqsr::cig_len(el);
    if (events > pilk::kMaxReadRows || rp > pilk::kMaxReadRows) return BQSR_ERR_UNSUPPORTED;
    P.X.evpre[c0 + e] = (uint32_t)events;
    P.X.readpre[c0 + e] = (uint32_t)rp;
    P.X.refpre[c0 + e] = ro;
    if (op == BQSR_CIGAR_M) {
      for (int64_t b = 0; b < len; ++b) {
        while (j < n_ent && (int64_t)(ent[j] >> 6) < ro) ++j;
        const bool hit = j < n_ent && (int64_t)(ent[j] >> 6) == ro;
        if (!hit && ro < span) {  // isMatch: the event, then baseFromSequence for the reference base
          if (no_name || no_rest || !has_seq) return BQSR_ERR_NULL_FIELD;
          if (rp >= ls || base5(pilk::base_index(R.seq[s0 + rp])) == kNoBase) return BQSR_ERR_PILEUP;
        } else if (hit && !(ent[j] & 32u)) {  // a mismatch: readName, baseFromSequence, the rest, the MD's base
          if (no_name || !has_seq) return BQSR_ERR_NULL_FIELD;
          if (rp >= ls || base5(pilk::base_index(R.seq[s0 + rp])) == kNoBase) return BQSR_ERR_PILEUP;
          if (no_rest) return BQSR_ERR_NULL_FIELD;
          if (base5((int)(ent[j] & 31u)) == kNoBase) return BQSR_ERR_PILEUP;
        } else {
          return BQSR_ERR_PILEUP;  // neither match nor mismatch: a delete there, or the MD has ended
        }
        ++rp;
        ++ro;
      }
      events += len;
    } else if (op == BQSR_CIGAR_D) {
      for (int64_t b = 0; b < len; ++b) {
        while (j < n_ent && (int64_t)(ent[j] >> 6) < ro) ++j;
        if (!(j < n_ent && (int64_t)(ent[j] >> 6) == ro && (ent[j] & 32u))) return BQSR_ERR_PILEUP;
        if (no_name || no_rest) return BQSR_ERR_NULL_FIELD;
        if (base5((int)(ent[j] & 31u)) == kNoBase) return BQSR_ERR_PILEUP;
        ++ro;
      }
      events += len;
    } else if (op == BQSR_CIGAR_I) {  // one event per element, carrying the whole sequence
      if (no_name || !has_seq || no_rest) return BQSR_ERR_NULL_FIELD;
      rp += len;
      events += 1;
    } else {
      if (op == BQSR_CIGAR_S || op == BQSR_CIGAR_EQ || op == BQSR_CIGAR_X) rp += len;  // consumesReadBases
      if (bqsr::consumes_ref(op)) ro += len;
    }
  }
  if (events > pilk::kMaxReadRows || rp > pilk::kMaxReadRows) return BQSR_ERR_UNSUPPORTED;
  *events_out = (uint64_t)events;
  *ro_out = ro;
  return 0;
}

extern "C" __global__ void __launch_bounds__(kThreads) mp_walk(WalkParams P) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < P.nk; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = P.kidx[k];
    const uint32_t f = P.A.R.flags[r];
    const int32_t id = P.A.ref_id[r];
    uint64_t events = 0;
    int64_t ro = 0;
    int st = 0;
    bool seg = true;
    // foreach: referenceId and start are unboxed before anything else
    if (id < 0 || !(f & BQSR_F_HAS_START)) {
      st = BQSR_ERR_NULL_FIELD;
      P.X.md_n[k] = 0;
    } else if (P.A.ref_name[r] >= P.A.n_names) {  // (a caller's name table shorter than its indices)
      st = BQSR_ERR_INVALID_ARG;
      P.X.md_n[k] = 0;
    } else {
      if (k > 0) {
        const int64_t rb = P.kidx[k - 1];
        seg = P.A.ref_id[rb] != id;
        if (!seg && (P.A.R.flags[rb] & BQSR_F_HAS_START) && P.A.R.start[r] < P.A.R.start[rb])
          atomicMin(P.unsorted, (unsigned long long)r);
      }
      st = walk_read(P, k, r, &events, &ro);
      // positions are key bits: none below 0
      if (!st && events && P.A.R.start[r] < 0) st = BQSR_ERR_UNSUPPORTED;
    }
    if (st) {
      events = 0;
      atomicMin(P.err, ((unsigned long long)r << 8) | (unsigned long long)st);
    }
    if (events) atomicMax(P.maxpos, (unsigned long long)(P.A.R.start[r] + ro));
    P.X.cnt[k] = events;
    P.X.segflag[k] = seg;
  }
}

// the largest i in [a, b] with rs[i] <= g (rs[a] <= g)
__device__ __forceinline__ int64_t last_le(const uint64_t* rs, int64_t a, int64_t b, uint64_t g) {
  while (a < b) {
    const int64_t m = (a + b + 1) >> 1;
    if (rs[m] <= g) a = m;
    else b = m - 1;
  }
  return a;
}

struct EmitParams {
  Reads A;
  Scratch X;
  const int64_t* kidx;
  const uint64_t* es;      // [nk + 1] first event of each kept read
  const uint32_t* segid1;  // [nk] inclusive scan of segflag: segment id + 1
  int64_t nk, n_ev;
  int pos_bits;
  uint64_t* key;
  uint64_t* val;  // kept-read index | char << 32 | reference-base code << 40
};

extern "C" __global__ void __launch_bounds__(kThreads) mp_emit(EmitParams P) {
  const pilk::Reads& R = P.A.R;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < P.n_ev; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = last_le(P.es, 0, P.nk - 1, (uint64_t)g);
    const int64_t r = P.kidx[k];
    const uint32_t w = (uint32_t)((uint64_t)g - P.es[k]);  // position in the walk
    const uint64_t c0 = R.cig_off[r];
    int64_t ea = 0, eb = (int64_t)(R.cig_off[r + 1] - c0) - 1;
    // the last element with evpre <= w: the one holding w (an element without
    // events shares the next one's prefix, and w is below every trailing one's)
    while (ea < eb) {
      const int64_t m = (ea + eb + 1) >> 1;
      if (P.X.evpre[c0 + m] <= w) ea = m;
      else eb = m - 1;
    }
    const uint32_t el = R.cig[c0 + ea], op = bqsr::cig_op(el);
    const uint32_t i = w - P.X.evpre[c0 + ea];  // index within the element
    const bool rev = R.flags[r] & BQSR_F_NEG_STRAND;
    uint32_t cls = kInsert, ch = 0, code = kNoBase;
    int64_t ro = P.X.refpre[c0 + ea];
    if (op != BQSR_CIGAR_I) {
      ro += i;
      const uint32_t* ent = P.X.mdent + R.md_off[r];
      int64_t a = 0, b = P.X.md_n[k];
      while (a < b) {  // first entry with offset >= ro
        const int64_t m = (a + b) >> 1;
        if ((int64_t)(ent[m] >> 6) < ro) a = m + 1;
        else b = m;
      }
      const bool hit = a < (int64_t)P.X.md_n[k] && (int64_t)(ent[a] >> 6) == ro;
      if (op == BQSR_CIGAR_D) {
        cls = kDelete;
        code = base5((int)(ent[a] & 31u));
      } else {
        const uint8_t c = R.seq[R.seq_off[r] + P.X.readpre[c0 + ea] + i];
        if (hit) {
          cls = kMismatch;
          code = base5((int)(ent[a] & 31u));
          ch = rev ? (uint32_t)(c + 32) : c;  // toLowerCase of A C T G N
        } else {
          cls = kMatch;
          code = base5(pilk::base_index(c));
          ch = rev ? ',' : '.';
        }
      }
    }
    const uint64_t pos = (uint64_t)(R.start[r] + ro);
    P.key[g] = ((uint64_t)(P.segid1[k] - 1) << (P.pos_bits + 2)) | (pos << 2) | cls;
    P.val[g] = (uint64_t)k | ((uint64_t)ch << 32) | ((uint64_t)code << 40);
  }
}

struct GroupParams {
  Reads A;
  const int64_t* kidx;
  const uint64_t* key;  // sorted
  const uint64_t* val;
  int64_t n_ev;
  uint32_t* head;    // [n_ev] 1: the event starts a line
  uint64_t* len;     // [n_ev + 1] rendered bytes of the event, then 0
  uint32_t* mask;    // [n_ev] 1 << reference-base code, 0: none
};

extern "C" __global__ void __launch_bounds__(kThreads) mp_heads(GroupParams P) {
  const pilk::Reads& R = P.A.R;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < P.n_ev; j += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t key = P.key[j], v = P.val[j];
    P.head[j] = j == 0 || (P.key[j - 1] >> 2) != (key >> 2);
    const uint32_t cls = (uint32_t)(key & 3), code = (uint32_t)(v >> 40) & 7u;
    uint64_t len = cls == kDelete ? 3 : 1;
    if (cls == kInsert) {
      const int64_t r = P.kidx[v & 0xFFFFFFFFull];
      const uint64_t ls = R.seq_off[r + 1] - R.seq_off[r];
      len = 1 + (uint64_t)digits(ls) + ls;
    }
    P.len[j] = len;
    P.mask[j] = code == kNoBase ? 0u : 1u << code;
    if (j == 0) P.len[P.n_ev] = 0;
  }
}

// first[l] = the first event of line l, first[n_lines] = n_ev
extern "C" __global__ void __launch_bounds__(kThreads) mp_first(const uint32_t* head, const uint32_t* line1,
                                                               int64_t n_ev, uint32_t* first) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n_ev; j += (int64_t)gridDim.x * blockDim.x) {
    if (head[j]) first[line1[j] - 1] = (uint32_t)j;
    if (j == n_ev - 1) first[line1[j]] = (uint32_t)n_ev;
  }
}

struct LineParams {
  Reads A;
  const int64_t* kidx;
  const uint64_t* key;
  const uint64_t* val;
  const uint32_t* first;     // [n_lines + 1]
  const uint64_t* evoff;     // [n_ev + 1] exclusive scan of len
  const uint32_t* linemask;  // [n_lines]
  const uint64_t* name_off;  // [n_names + 1]
  int64_t n_lines;
  int pos_bits;
  uint32_t* hdrlen;   // [n_lines]
  uint8_t* linebase;  // [n_lines] the reference base's character, '?' without
  uint64_t* linelen;  // [n_lines + 1], then 0
  unsigned long long* conflict;  // atomicMin of the line whose events disagree on the reference base
};

extern "C" __global__ void __launch_bounds__(kThreads) mp_lines(LineParams P) {
  for (int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; l < P.n_lines; l += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t j0 = P.first[l], j1 = P.first[l + 1];
    const uint64_t pos = (P.key[j0] >> 2) & ((1ull << P.pos_bits) - 1);
    const int32_t nm = P.A.ref_name[P.kidx[P.val[j0] & 0xFFFFFFFFull]];
    const uint32_t m = P.linemask[l];
    if (__popc(m) > 1) atomicMin(P.conflict, (unsigned long long)l);
    P.linebase[l] = m ? (uint8_t)kBaseChar[__ffs(m) - 1] : (uint8_t)'?';
    // "%s %s " name, position; the base; " " numReads " "
    const uint32_t h = (uint32_t)(P.name_off[nm + 1] - P.name_off[nm]) + 1 + digits(pos) + 1 + 1 + 1 +
                       digits(j1 - j0) + 1;
    P.hdrlen[l] = h;
    P.linelen[l] = h + (P.evoff[j1] - P.evoff[j0]) + 1;
    if (l == 0) P.linelen[P.n_lines] = 0;
  }
}

// the window of whole lines from line0 within `budget` bytes: out[0] = its end
// line, out[1] / out[2] = byte offsets of line0 and the end line, out[3] =
// byte offset of line0 + 1, out[4] / out[5] = first events of line0 and the
// end line
extern "C" __global__ void mp_window(const uint64_t* lineoff, const uint32_t* first, int64_t n_lines, int64_t line0,
                                     uint64_t budget, uint64_t* out) {
  if (blockIdx.x || threadIdx.x) return;
  const uint64_t b0 = lineoff[line0];
  int64_t a = line0, b = n_lines;
  while (a < b) {  // the largest l with lineoff[l] - b0 <= budget
    const int64_t m = (a + b + 1) >> 1;
    if (lineoff[m] - b0 <= budget) a = m;
    else b = m - 1;
  }
  out[0] = (uint64_t)a;
  out[1] = b0;
  out[2] = lineoff[a];
  out[3] = lineoff[line0 < n_lines ? line0 + 1 : line0];
  out[4] = first[line0];
  out[5] = first[a];
}

struct TextParams {
  Reads A;
  const int64_t* kidx;
  const uint64_t* key;
  const uint64_t* val;
  const uint32_t* line1;  // [n_ev] line id + 1
  const uint32_t* first;
  const uint64_t* evoff;
  const uint64_t* lineoff;
  const uint32_t* hdrlen;
  const uint8_t* linebase;
  const uint8_t* names;
  const uint64_t* name_off;
  int64_t e0, e1;   // the window's events
  uint64_t base0;   // byte offset of its first line
  uint64_t nbytes;  // its size
  int pos_bits;
  uint8_t* out;
};

extern "C" __global__ void __launch_bounds__(kThreads) mp_text(TextParams P) {
  const pilk::Reads& R = P.A.R;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  uint8_t* out = P.out;
  for (int64_t g0 = P.e0 + wave * 64; g0 < P.e1; g0 += waves * 64) {  // (the same trips in every lane)
    const int64_t j = g0 + lane;
    const bool live = j < P.e1;
    uint64_t o = 0;      // where this event's bytes go
    int64_t ins_r = -1;  // the read of an insertion
    if (live) {
      const uint64_t key = P.key[j], v = P.val[j];
      const int64_t l = (int64_t)P.line1[j] - 1;
      const uint32_t j0 = P.first[l], j1 = P.first[l + 1];
      const uint64_t lo = P.lineoff[l] - P.base0;
      const uint32_t h = P.hdrlen[l];
      const uint32_t cls = (uint32_t)(key & 3);
      o = lo + h + (P.evoff[j] - P.evoff[j0]);
      const uint64_t end = P.lineoff[l + 1] - P.base0;  // one past the newline
      if (end <= P.nbytes) {                             // (always: the window is whole lines)
        if (cls == kMatch || cls == kMismatch) {
          out[o] = (uint8_t)(v >> 32);
        } else if (cls == kDelete) {
          out[o] = '-';
          out[o + 1] = '1';
          out[o + 2] = P.linebase[l];
        } else {
          ins_r = P.kidx[v & 0xFFFFFFFFull];
        }
        if ((uint32_t)j == j0) {  // the header
          const int32_t nm = P.A.ref_name[P.kidx[v & 0xFFFFFFFFull]];
          const uint64_t na = P.name_off[nm], nn = P.name_off[nm + 1] - na;
          uint64_t p = lo;
          for (uint64_t t = 0; t < nn; ++t) out[p + t] = P.names[na + t];
          p += nn;
          out[p++] = ' ';
          const uint64_t pos = (key >> 2) & ((1ull << P.pos_bits) - 1);
          int nd = digits(pos);
          put_dec(out, p, pos, nd);
          p += (uint64_t)nd;
          out[p++] = ' ';
          out[p++] = P.linebase[l];
          out[p++] = ' ';
          nd = digits(j1 - j0);
          put_dec(out, p, j1 - j0, nd);
          p += (uint64_t)nd;
          out[p] = ' ';
        }
        if ((uint32_t)j == j1 - 1) out[end - 1] = '\n';
      }
    }
    // insertions: "+", the read's length, the whole read, by all 64 lanes
    uint64_t todo = __builtin_amdgcn_ballot_w64(ins_r >= 0);
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint64_t so = ((uint64_t)(uint32_t)__shfl((int)(o >> 32), src) << 32) | (uint32_t)__shfl((int)o, src);
      const int64_t sr = (int64_t)(((uint64_t)(uint32_t)__shfl((int)((uint64_t)ins_r >> 32), src) << 32) |
                                   (uint32_t)__shfl((int)ins_r, src));
      const uint64_t s0 = R.seq_off[sr], ls = R.seq_off[sr + 1] - s0;
      const int nd = digits(ls);
      if (so + 1 + (uint64_t)nd + ls <= P.nbytes) {
        if (lane == 0) {
          out[so] = '+';
          put_dec(out, so + 1, ls, nd);
        }
        uint8_t* dst = out + so + 1 + (uint64_t)nd;
        for (uint64_t t = (uint64_t)lane; t < ls; t += 64) dst[t] = R.seq[s0 + t];
      }
    }
  }
}

}  // namespace mpk

namespace {

struct MpState {
  DevBuf keep, kpos, kidx, evpre, readpre, refpre, mdent, cnt, es, md_n, segflag, segid1, key_a, key_b, val_a, val_b, head,
      line1, len, evoff, mask, first, linemask, hdrlen, linebase, linelen, lineoff, temp, names, name_off, out, small;
  uint64_t *key = nullptr, *val = nullptr;  // the sorted ones
  int64_t nk = 0, n_ev = 0, n_lines = 0, text_bytes = 0;
  int pos_bits = 1;
  bool prepared = false;
  StageClock<8> clock;
};

// the stages of the calling thread's last prepare / text calls (mpileup.KERNELS), and the clock's marks: the one
// after emit starts sort, the one after sort starts group
enum { MP_WALK, MP_EMIT, MP_SORT, MP_GROUP, MP_TEXT, MP_STAGES };
enum { MP_WALK_0, MP_WALK_1, MP_EMIT_0, MP_SORT_0, MP_GROUP_0, MP_GROUP_1, MP_TEXT_0, MP_TEXT_1 };
thread_local double g_mpileup_ms[MP_STAGES] = {0.0, 0.0, 0.0, 0.0, 0.0};

struct MpView {
  mpk::Reads A;
  int64_t n_reads, cig_ops, md_bytes;
  std::vector<std::string> names;
};

const char* mp_what(int status) {
  switch (status) {
    case BQSR_ERR_NULL_FIELD:
      return "a null referenceId, start, readName, mapq, qual, sequence or referenceName (the reference throws a "
             "NullPointerException)";
    case BQSR_ERR_MD_PARSE:
      return "an MD tag MdTag.apply rejects";
    case BQSR_ERR_PILEUP:
      return "an exception inside readToPileups (a base outside A C T G N in the sequence or the MD, a sequence "
             "shorter than the CIGAR, or CIGAR and MD disagreeing)";
    case BQSR_ERR_INVALID_ARG:
      return "a referenceName index beyond the names given";
    default:
      return "beyond the device path's limits (a start below 0, a mismatch or deleted base 2^26 or more positions "
             "after the read's start, or 2^31 or more events or read bases in one read)";
  }
}

bqsr_status mp_prepare(bqsr_context* ctx, MpState& A, const MpView& V, hipStream_t s, bqsr_mpileup_sizes* out) {
  using namespace mpk;
  A.prepared = false;
  A.nk = A.n_ev = A.n_lines = A.text_bytes = 0;
  *out = bqsr_mpileup_sizes{0, 0, 0, 0};
  for (double& t : g_mpileup_ms) t = 0.0;
  const int64_t n = V.n_reads;
  if (n > (int64_t)INT32_MAX)
    return fail(BQSR_ERR_UNSUPPORTED, "mpileup: more than 2^31 - 1 reads in one job");
  if (n == 0) {
    A.prepared = true;
    return ok();
  }
  bqsr_status e;
  auto need = [](DevBuf& b, auto** p, size_t count, const char* what) {
    return dev_need(b, p, count, "mpileup", what);
  };
  auto prim = [&](auto&& call) { return dev_prim(A.temp, "mpileup", call); };
  auto grid = [&](int64_t items) { return pileup_job_grid(ctx, items, kThreads); };
  // ---- the name table ----
  {
    std::vector<uint8_t> blob;
    std::vector<uint64_t> off{0};
    for (const std::string& nm : V.names) {
      blob.insert(blob.end(), nm.begin(), nm.end());
      off.push_back(blob.size());
    }
    uint8_t* dn;
    uint64_t* doff;
    if ((e = need(A.names, &dn, blob.size(), "reference names")) || (e = need(A.name_off, &doff, off.size(), "reference names")))
      return e;
    if (!blob.empty()) HIP_TRY(hipMemcpyAsync(dn, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(doff, off.data(), off.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (the host vectors go out of scope)
  }
  // ---- the kept reads ----
  uint32_t *keep, *kpos;
  int64_t* kidx;
  unsigned long long* small;  // err, unsorted, maxpos, conflict, then mp_window's six words
  if ((e = need(A.keep, &keep, (size_t)n + 1, "reads")) || (e = need(A.kpos, &kpos, (size_t)n + 1, "reads")) ||
      (e = need(A.kidx, &kidx, (size_t)n, "reads")) || (e = need(A.small, &small, 16, "status words")))
    return e;
  HIP_TRY(hipMemsetAsync(small, 0xFF, 16 * 8, s));
  HIP_TRY(hipMemsetAsync(small + 2, 0, 8, s));
  HIP_TRY(A.clock.mark(MP_WALK_0, s));
  JOB_TRY(launch(mp_keep, grid(n), kThreads, s, V.A, n, keep));
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::exclusive_scan(t, b, keep, kpos, (uint32_t)0, (size_t)n + 1, rocprim::plus<uint32_t>(), s);
       })))
    return e;
  JOB_TRY(launch(mp_compact, grid(n), kThreads, s, keep, kpos, n, kidx));
  uint32_t nk32 = 0;
  HIP_TRY(hipMemcpyAsync(&nk32, kpos + n, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int64_t nk = nk32;
  A.nk = nk;
  out->n_reads = nk;
  if (nk == 0) {
    A.prepared = true;
    return ok();
  }
  // ---- walk ----
  Scratch X{};
  uint64_t* es;
  uint32_t* segid1;
  const size_t nc = (size_t)V.cig_ops, nm = (size_t)V.md_bytes, K = (size_t)nk;
  if ((e = need(A.evpre, &X.evpre, nc, "CIGAR elements")) || (e = need(A.readpre, &X.readpre, nc, "CIGAR elements")) ||
      (e = need(A.refpre, &X.refpre, nc, "CIGAR elements")) || (e = need(A.mdent, &X.mdent, nm, "MD entries")) ||
      (e = need(A.cnt, &X.cnt, K + 1, "kept reads")) || (e = need(A.es, &es, K + 1, "kept reads")) ||
      (e = need(A.md_n, &X.md_n, K, "kept reads")) || (e = need(A.segflag, &X.segflag, K, "kept reads")) ||
      (e = need(A.segid1, &segid1, K, "kept reads")))
    return e;
  HIP_TRY(hipMemsetAsync(X.cnt + nk, 0, 8, s));
  WalkParams W{V.A, X, kidx, nk, small, small + 1, small + 2};
  JOB_TRY(launch(mp_walk, grid(nk), kThreads, s, W));
  HIP_TRY(A.clock.mark(MP_WALK_1, s));
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::exclusive_scan(t, b, X.cnt, es, (uint64_t)0, K + 1, rocprim::plus<uint64_t>(), s);
       })) ||
      (e = prim([&](void* t, size_t& b) {
         return rocprim::inclusive_scan(t, b, X.segflag, segid1, K, rocprim::plus<uint32_t>(), s);
       })))
    return e;
  unsigned long long st3[3] = {~0ull, ~0ull, 0};
  uint64_t total = 0;
  uint32_t n_seg = 0;
  HIP_TRY(hipMemcpyAsync(st3, small, 24, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&total, es + nk, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&n_seg, segid1 + (nk - 1), 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  A.clock.add(g_mpileup_ms[MP_WALK], MP_WALK_0, MP_WALK_1);
  if (st3[0] != ~0ull) {
    const int status = (int)(st3[0] & 0xFF);
    const int64_t read = (int64_t)(st3[0] >> 8);
    return fail((bqsr_status)status, "mpileup: read " + std::to_string(read) + ": " + mp_what(status), read);
  }
  if (st3[1] != ~0ull) {
    const int64_t read = (int64_t)st3[1];
    return fail(BQSR_ERR_UNSORTED, "mpileup: read " + std::to_string(read) + " starts before the kept read in front of "
                "it on the same reference: pileups need reads sorted by position (transform -sort_reads)", read);
  }
  if (total > (uint64_t)INT32_MAX)
    return fail(BQSR_ERR_UNSUPPORTED, "mpileup: more than 2^31 - 1 events in one job");
  const int64_t m = (int64_t)total;
  A.n_ev = m;
  out->n_events = m;
  if (m == 0) {
    A.prepared = true;
    return ok();
  }
  const int pos_bits = std::max(1, bits_of((uint64_t)st3[2]));
  const int key_bits = 2 + pos_bits + bits_of((uint64_t)n_seg - 1);
  if (key_bits > 64)
    return fail(BQSR_ERR_UNSUPPORTED, "mpileup: segment, position and class need " + std::to_string(key_bits) +
                " key bits, more than 64");
  A.pos_bits = pos_bits;
  // ---- emit, sort ----
  const size_t M = (size_t)m;
  uint64_t *key_a, *key_b, *val_a, *val_b;
  if ((e = need(A.key_a, &key_a, M, "events")) || (e = need(A.key_b, &key_b, M, "events")) ||
      (e = need(A.val_a, &val_a, M, "events")) || (e = need(A.val_b, &val_b, M, "events")))
    return e;
  EmitParams E{V.A, X, kidx, es, segid1, nk, m, pos_bits, key_a, val_a};
  HIP_TRY(A.clock.mark(MP_EMIT_0, s));
  JOB_TRY(launch(mp_emit, grid(m), kThreads, s, E));
  HIP_TRY(A.clock.mark(MP_SORT_0, s));
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::radix_sort_pairs(t, b, key_a, key_b, val_a, val_b, M, 0, (unsigned)key_bits, s);
       })))
    return e;
  HIP_TRY(A.clock.mark(MP_GROUP_0, s));
  A.key = key_b;
  A.val = val_b;
  // ---- group ----
  uint32_t *head, *line1, *mask, *first, *linemask, *hdrlen;
  uint64_t *len, *evoff, *linelen, *lineoff;
  uint8_t* linebase;
  if ((e = need(A.head, &head, M + 1, "events")) || (e = need(A.line1, &line1, M, "events")) ||
      (e = need(A.len, &len, M + 1, "events")) || (e = need(A.evoff, &evoff, M + 1, "events")) ||
      (e = need(A.mask, &mask, M, "events")) || (e = need(A.first, &first, M + 1, "events")))
    return e;
  GroupParams G{V.A, kidx, key_b, val_b, m, head, len, mask};
  JOB_TRY(launch(mp_heads, grid(m), kThreads, s, G));
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::inclusive_scan(t, b, head, line1, M, rocprim::plus<uint32_t>(), s);
       })) ||
      (e = prim([&](void* t, size_t& b) {
         return rocprim::exclusive_scan(t, b, len, evoff, (uint64_t)0, M + 1, rocprim::plus<uint64_t>(), s);
       })))
    return e;
  uint32_t nl32 = 0;
  HIP_TRY(hipMemcpyAsync(&nl32, line1 + (m - 1), 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int64_t nl = nl32;
  const size_t NL = (size_t)nl;
  if ((e = need(A.linemask, &linemask, NL + 1, "lines")) || (e = need(A.hdrlen, &hdrlen, NL, "lines")) ||
      (e = need(A.linebase, &linebase, NL, "lines")) || (e = need(A.linelen, &linelen, NL + 1, "lines")) ||
      (e = need(A.lineoff, &lineoff, NL + 1, "lines")))
    return e;
  JOB_TRY(launch(mp_first, grid(m), kThreads, s, head, line1, m, first));
  // per line the OR of its events' reference-base bits (head is free: the unique keys go there, the count after them)
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::reduce_by_key(t, b, line1, mask, M, head, linemask, linemask + nl, mpk::BitOr(),
                                       rocprim::equal_to<uint32_t>(), s);
       })))
    return e;
  LineParams LP{V.A, kidx, key_b, val_b, first, evoff, linemask, (const uint64_t*)A.name_off.p, nl, pos_bits,
                hdrlen, linebase, linelen, small + 3};
  JOB_TRY(launch(mp_lines, grid(nl), kThreads, s, LP));
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::exclusive_scan(t, b, linelen, lineoff, (uint64_t)0, NL + 1, rocprim::plus<uint64_t>(), s);
       })))
    return e;
  HIP_TRY(A.clock.mark(MP_GROUP_1, s));
  unsigned long long conflict = ~0ull;
  uint64_t bytes = 0;
  HIP_TRY(hipMemcpyAsync(&conflict, small + 3, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&bytes, lineoff + nl, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  A.clock.add(g_mpileup_ms[MP_EMIT], MP_EMIT_0, MP_SORT_0);
  A.clock.add(g_mpileup_ms[MP_SORT], MP_SORT_0, MP_GROUP_0);
  A.clock.add(g_mpileup_ms[MP_GROUP], MP_GROUP_0, MP_GROUP_1);
  if (conflict != ~0ull) {  // name the reference and the position
    uint32_t j0 = 0;
    uint64_t key = 0, val = 0;
    int64_t r = 0;
    int32_t nm_i = -1;
    HIP_TRY(hipMemcpy(&j0, first + conflict, 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&key, key_b + j0, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&val, val_b + j0, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&r, kidx + (val & 0xFFFFFFFFull), 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&nm_i, V.A.ref_name + r, 4, hipMemcpyDeviceToHost));
    const int64_t pos = (int64_t)((key >> 2) & ((1ull << pos_bits) - 1));
    const std::string nm_s = nm_i >= 0 && nm_i < (int32_t)V.names.size() ? V.names[(size_t)nm_i] : std::string("?");
    return fail(BQSR_ERR_REFERENCE_CONFLICT, "mpileup: reference " + nm_s + " position " + std::to_string(pos) +
                ": the reads' MD tags and bases disagree on the reference base (the reference's AssertionError)", pos);
  }
  A.n_lines = nl;
  A.text_bytes = (int64_t)bytes;
  out->n_lines = nl;
  out->text_bytes = (int64_t)bytes;
  A.prepared = true;
  return ok();
}

bqsr_status mp_text_call(bqsr_context* ctx, MpState& A, const MpView& V, int64_t line0, int64_t budget, char* dst,
                         hipStream_t s, int64_t* n_lines, int64_t* n_bytes, const char* who) {
  using namespace mpk;
  if (!A.prepared) return fail(BQSR_ERR_INVALID_ARG, std::string(who) + " before its prepare call");
  if (line0 < 0 || line0 > A.n_lines || budget < 0)
    return fail(BQSR_ERR_INVALID_ARG, std::string(who) + ": line0 or the budget out of range");
  *n_lines = 0;
  *n_bytes = 0;
  g_mpileup_ms[MP_TEXT] = 0.0;
  if (line0 == A.n_lines) return ok();
  unsigned long long* small = (unsigned long long*)A.small.p;
  uint64_t* win = (uint64_t*)(small + 8);
  JOB_TRY(launch(mp_window, 1, 64, s, (const uint64_t*)A.lineoff.p, (const uint32_t*)A.first.p, A.n_lines, line0,
                 (uint64_t)budget, win));
  uint64_t w[6];
  HIP_TRY(hipMemcpyAsync(w, win, sizeof w, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int64_t l1 = (int64_t)w[0];
  if (l1 == line0)
    return fail(BQSR_ERR_INVALID_ARG, std::string(who) + ": line " + std::to_string(line0) + " takes " +
                std::to_string(w[3] - w[1]) + " bytes, more than the budget of " + std::to_string(budget));
  const uint64_t nbytes = w[2] - w[1];
  if (!dst) return fail(BQSR_ERR_INVALID_ARG, std::string(who) + ": null destination");
  uint8_t* out;
  bqsr_status e;
  if ((e = dev_need(A.out, &out, (size_t)nbytes + 64, "mpileup", "text window"))) return e;
  TextParams T{V.A, (const int64_t*)A.kidx.p, A.key, A.val, (const uint32_t*)A.line1.p, (const uint32_t*)A.first.p,
               (const uint64_t*)A.evoff.p, (const uint64_t*)A.lineoff.p, (const uint32_t*)A.hdrlen.p,
               (const uint8_t*)A.linebase.p, (const uint8_t*)A.names.p, (const uint64_t*)A.name_off.p,
               (int64_t)w[4], (int64_t)w[5], w[1], nbytes, A.pos_bits, out};
  HIP_TRY(A.clock.mark(MP_TEXT_0, s));
  JOB_TRY(launch(mp_text, pileup_job_grid(ctx, T.e1 - T.e0, kThreads), kThreads, s, T));
  HIP_TRY(A.clock.mark(MP_TEXT_1, s));
  HIP_TRY(hipMemcpyAsync(dst, out, (size_t)nbytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  A.clock.add(g_mpileup_ms[MP_TEXT], MP_TEXT_0, MP_TEXT_1);
  *n_lines = l1 - line0;
  *n_bytes = (int64_t)nbytes;
  return ok();
}

MpView mp_view(const bqsr_sam* s) {
  MpView V{};
  V.A = mpk::Reads{pileup_view(s).R, s->raw_flag, s->sq_id, s->ref, nullptr, (int32_t)s->ref_names.size()};
  V.n_reads = s->n_reads;
  V.cig_ops = s->cig_ops;
  V.md_bytes = s->md_bytes;
  V.names = s->ref_names;
  return V;
}

MpView mp_view(const bqsr_arrow* a, const PileupState& P, const std::vector<std::string>& names) {
  MpView V{};
  V.A = mpk::Reads{pileup_view(a, P).R, nullptr, a->sq, a->ref, a->name_valid, (int32_t)names.size()};
  V.n_reads = a->n;
  V.cig_ops = a->cig_ops;
  V.md_bytes = a->md_bytes;
  V.names = names;
  return V;
}

struct MpArrowNames {
  std::vector<std::string> names;
};

}  // namespace

extern "C" {

bqsr_status bqsr_sam_mpileup_prepare(bqsr_context* ctx, bqsr_sam* s, void* stream, bqsr_mpileup_sizes* out) {
  if (!ctx || !s || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_mpileup_prepare: bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  return mp_prepare(ctx, *job_state<MpState>(s->mpileup), mp_view(s), S(stream), out);
}

bqsr_status bqsr_sam_mpileup_text(bqsr_context* ctx, bqsr_sam* s, int64_t line0, int64_t budget, char* dst, void* stream,
                                  int64_t* n_lines, int64_t* n_bytes) {
  if (!ctx || !s || !n_lines || !n_bytes) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_mpileup_text: bad arguments");
  if (!s->mpileup) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_mpileup_text before bqsr_sam_mpileup_prepare");
  HIP_TRY(hipSetDevice(ctx->device));
  return mp_text_call(ctx, *job_state<MpState>(s->mpileup), mp_view(s), line0, budget, dst, S(stream), n_lines, n_bytes,
                      "bqsr_sam_mpileup_text");
}

bqsr_status bqsr_arrow_mpileup_prepare(bqsr_context* ctx, bqsr_arrow* a, const int64_t* chunk_reads,
                                       const int32_t* const* mapq, const uint8_t* const* mapq_validity,
                                       int32_t n_chunks, const char* const* ref_names, int32_t n_ref_names,
                                       void* stream, bqsr_mpileup_sizes* out) {
  if (!ctx || !a || !out || n_chunks < 0 || (n_chunks && (!chunk_reads || !mapq || !mapq_validity)) ||
      n_ref_names < 0 || (n_ref_names && !ref_names))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_mpileup_prepare: bad arguments");
  for (int32_t i = 0; i < n_ref_names; ++i)
    if (!ref_names[i]) return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_mpileup_prepare: a null reference name");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  PileupState& P = *job_state<PileupState>(a->pileup);
  if (n_chunks) {
    const bqsr_status e = pileup_arrow_mapq(ctx, a, P, chunk_reads, mapq, mapq_validity, n_chunks, s,
                                            "bqsr_arrow_mpileup_prepare");
    if (e != BQSR_OK) return e;
  }
  if (!a->mpileup_names) a->mpileup_names = std::shared_ptr<void>(new MpArrowNames, [](void* p) { delete (MpArrowNames*)p; });
  MpArrowNames& N = *(MpArrowNames*)a->mpileup_names.get();
  N.names.assign(ref_names, ref_names + n_ref_names);
  return mp_prepare(ctx, *job_state<MpState>(a->mpileup), mp_view(a, P, N.names), s, out);
}

bqsr_status bqsr_arrow_mpileup_text(bqsr_context* ctx, bqsr_arrow* a, int64_t line0, int64_t budget, char* dst,
                                    void* stream, int64_t* n_lines, int64_t* n_bytes) {
  if (!ctx || !a || !n_lines || !n_bytes) return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_mpileup_text: bad arguments");
  if (!a->mpileup || !a->mpileup_names)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_mpileup_text before bqsr_arrow_mpileup_prepare");
  HIP_TRY(hipSetDevice(ctx->device));
  MpArrowNames& N = *(MpArrowNames*)a->mpileup_names.get();
  return mp_text_call(ctx, *job_state<MpState>(a->mpileup), mp_view(a, *job_state<PileupState>(a->pileup), N.names),
                      line0, budget, dst, S(stream), n_lines, n_bytes, "bqsr_arrow_mpileup_text");
}

bqsr_status bqsr_mpileup_kernel_times(double* ms5) {
  if (!ms5) return fail(BQSR_ERR_INVALID_ARG, "bqsr_mpileup_kernel_times: null");
  for (int k = 0; k < MP_STAGES; ++k) ms5[k] = g_mpileup_ms[k];
  return BQSR_OK;
}

}  // extern "C"
