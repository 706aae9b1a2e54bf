// `adam aggregate_pileups` / `reads2ref -aggregate` on the device
// (include/adam_sam.h: bqsr_pileup_agg_*): PileupAggregator.aggregate
// (core/rdd/PileupAggregator.scala:25-219) over ADAMPileup rows kept in HBM as
// columns, under the two orders the header declares: rows fold in input row
// order, groups come out in key order.
//
// A handle holds every added row: the numeric and Base columns, one u16 of
// validity bits per row (bit k = column k present, the k* constants below), an
// int32 sample code and an int32 record-group code.  Rows come from the host
// (bqsr_pileup_agg_add_host) or straight from pileup.hip's emit pass, which
// writes its columns at the handle's next free row (bqsr_*_pileup_agg_add).
//
// bqsr_pileup_agg_run:
//   agg_keys      a lane per row: the 64-bit minor key readBase | rangeOffset |
//       sample, each component with a null slot below its values; the nulls
//       that throw in every row, the lowest offending row kept by atomicMin on
//       an error word (row << 8 | status, as pileup.hip) -- one word for what
//       throws while grouping, one for what the folds throw, which the scans
//       and emit add to; the OR and the AND of every key, which give the bits
//       the sort has to look at.
//   (sort)        stable rocprim::radix_sort_pairs, LSD over three keys --
//       minor, position, referenceId -- each over the bits in which its keys
//       differ; the payload is the u32 row index.
//   agg_heads     a group starts where the full key differs from the sorted
//       row before it.
//   agg_scan1_*   a segmented inclusive scan of the plain monoids (count, soft-
//       clip, reverse-strand and record-group-change sums mod 2^32, readStart
//       min, readEnd max) together with the running number of heads.
//   agg_scan2_*   the reference's fold M <- M * C + m_k * c_k is serial as
//       written, but with C_{k-1} known from the first scan every row is an
//       affine map x -> x * A + B over Z / 2^32 (a head: A = 0, B = m_1; a
//       later row: A = C_{k-1}, B = m_k * c_k), and affine maps compose
//       associatively: (A1, B1) then (A2, B2) is (A1 * A2, B1 * A2 + B2).  A
//       head's A = 0 cuts the segments by itself.  One scan of (A, B_map,
//       B_sanger) gives (M, S) at every group's last row.
//       Both scans run per 256-row tile: shuffles across the 64 lanes, the four
//       wave totals through LDS, and one carry per tile, scanned by a single
//       workgroup between the passes, so a group may span any number of tiles.
//   agg_emit      a lane per group, a wavefront per 64 consecutive groups:
//       copied fields from the group's first row, the Java divisions, the
//       validity words by ballot.
//
// Included by bqsr_capi.cpp after pileup.hip.

namespace pagk {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTopThreads = 1024;
// validity bits of a row
enum : uint32_t {
  kRef = 0, kPos, kRoff, kRlen, kRefBase, kReadBase, kSanger, kMapq, kSoft, kRev, kCount, kRstart, kRend, kSample,
  kCols
};
constexpr uint32_t kKeyRow = (1u << kRef) | (1u << kPos);                          // unboxed while grouping
constexpr uint32_t kEveryRow = (1u << kSanger) | (1u << kMapq) | (1u << kCount);  // unboxed by every fold
constexpr uint32_t kDeepRow = (1u << kSoft) | (1u << kRev) | (1u << kRstart) | (1u << kRend);
// minor key: readBase 9 bits | rangeOffset 33 bits | sample 22 bits, 0 = null in each
constexpr int kSampleBits = 22, kRoffBits = 33;
constexpr int32_t kMaxSample = (1 << kSampleBits) - 2;

struct Rows {
  int32_t* reference_id;
  int64_t* position;
  int32_t *range_offset, *range_length;
  uint8_t *reference_base, *read_base;
  int32_t *sanger, *mapq, *soft, *rev, *count;
  int64_t *read_start, *read_end;
  int32_t *sample, *rg;
  int32_t* name;  // the caller's code of the row's readName (reads: the read's ordinal)
  uint16_t* mask;
};

struct PackHost {
  Rows R;
  int64_t base, n;
  const uint8_t* bm[kCols];  // Arrow bitmaps of this add's rows (null: all valid)
  uint32_t present;          // columns given at all
  int32_t implicit_names;    // no name codes given: a row's code is its index in the handle
};

extern "C" __global__ void __launch_bounds__(kThreads) agg_pack_host(PackHost P) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P.n; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t m = 0;
    for (uint32_t k = 0; k < kCols; ++k)
      if (((P.present >> k) & 1u) && (!P.bm[k] || ((P.bm[k][i >> 3] >> (i & 7)) & 1u))) m |= 1u << k;
    P.R.mask[P.base + i] = (uint16_t)m;
    if (P.implicit_names) P.R.name[P.base + i] = (int32_t)(P.base + i);
  }
}

struct PackReads {
  Rows R;
  int64_t base, n, r0, name_base;
  const int32_t* read;  // the emit pass's read column: the row's read, counted from r0
  const uint64_t *v_range, *v_reference_base, *v_read_base, *v_mapq;
  const int32_t* ref_id;               // per read of the parse, -1 null
  const int32_t *sample_code, *rg_code;  // per read of the range; a negative sample code: null
};

extern "C" __global__ void __launch_bounds__(kThreads) agg_pack_reads(PackReads P) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t rd = P.read[i];
    const int32_t ref = P.ref_id[P.r0 + rd], sm = P.sample_code[rd];
    auto bit = [&](const uint64_t* w) -> uint32_t { return (uint32_t)((w[i >> 6] >> (i & 63)) & 1u); };
    uint32_t m = (1u << kPos) | (1u << kSanger) | (1u << kSoft) | (1u << kRev) | (1u << kCount) | (1u << kRstart) |
                 (1u << kRend);
    if (ref >= 0) m |= 1u << kRef;
    if (sm >= 0) m |= 1u << kSample;
    if (bit(P.v_range)) m |= (1u << kRoff) | (1u << kRlen);
    if (bit(P.v_reference_base)) m |= 1u << kRefBase;
    if (bit(P.v_read_base)) m |= 1u << kReadBase;
    if (bit(P.v_mapq)) m |= 1u << kMapq;
    const int64_t g = P.base + i;
    P.R.reference_id[g] = ref >= 0 ? ref : 0;
    P.R.sample[g] = sm >= 0 ? sm : 0;
    P.R.rg[g] = P.rg_code[rd];
    P.R.name[g] = (int32_t)(P.name_base + rd);
    P.R.count[g] = 1;
    P.R.mask[g] = (uint16_t)m;
  }
}

__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
  for (int d = 32; d; d >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, d);
  return v;
}
__device__ __forceinline__ uint64_t wave_and(uint64_t v) {
  for (int d = 32; d; d >>= 1) v &= (uint64_t)__shfl_xor((unsigned long long)v, d);
  return v;
}
__device__ __forceinline__ uint64_t key_position(int64_t p) { return (uint64_t)p ^ 0x8000000000000000ull; }
__device__ __forceinline__ uint64_t key_reference(int32_t r) { return (uint64_t)((uint32_t)r ^ 0x80000000u); }

struct KeysParams {
  Rows R;
  int64_t n;
  uint64_t* minor;
  unsigned long long* err;   // atomicMin of row << 8 | status: what stops the run before the groups exist
  unsigned long long* fold;  // the same for what the folds throw (with the scans' and emit's)
  unsigned long long* stat;  // OR of the minor, position, referenceId keys, then their ANDs
};

extern "C" __global__ void __launch_bounds__(kThreads) agg_keys(KeysParams P) {
  uint64_t o0 = 0, o1 = 0, o2 = 0, a0 = ~0ull, a1 = ~0ull, a2 = ~0ull;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P.n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t m = P.R.mask[i];
    const int32_t sm = P.R.sample[i];
    int st = 0;
    if ((m & kKeyRow) != kKeyRow) st = BQSR_ERR_NULL_FIELD;
    else if (((m >> kSample) & 1u) && (sm < 0 || sm > kMaxSample)) st = BQSR_ERR_UNSUPPORTED;
    if (st) atomicMin(P.err, ((unsigned long long)i << 8) | (unsigned long long)st);
    if ((m & kEveryRow) != kEveryRow)
      atomicMin(P.fold, ((unsigned long long)i << 8) | (unsigned long long)BQSR_ERR_NULL_FIELD);
    const uint64_t kb = ((m >> kReadBase) & 1u) ? (uint64_t)P.R.read_base[i] + 1 : 0;
    const uint64_t ko = ((m >> kRoff) & 1u) ? (uint64_t)((uint32_t)P.R.range_offset[i] ^ 0x80000000u) + 1 : 0;
    const uint64_t ks = ((m >> kSample) & 1u) ? ((uint64_t)(uint32_t)sm + 1) & ((1ull << kSampleBits) - 1) : 0;
    const uint64_t k0 = (kb << (kRoffBits + kSampleBits)) | (ko << kSampleBits) | ks;
    const uint64_t k1 = key_position(P.R.position[i]), k2 = key_reference(P.R.reference_id[i]);
    P.minor[i] = k0;
    o0 |= k0, o1 |= k1, o2 |= k2;
    a0 &= k0, a1 &= k1, a2 &= k2;
  }
  o0 = wave_or(o0), o1 = wave_or(o1), o2 = wave_or(o2);
  a0 = wave_and(a0), a1 = wave_and(a1), a2 = wave_and(a2);
  if ((threadIdx.x & 63) == 0) {
    atomicOr(P.stat + 0, (unsigned long long)o0);
    atomicOr(P.stat + 1, (unsigned long long)o1);
    atomicOr(P.stat + 2, (unsigned long long)o2);
    atomicAnd(P.stat + 3, (unsigned long long)a0);
    atomicAnd(P.stat + 4, (unsigned long long)a1);
    atomicAnd(P.stat + 5, (unsigned long long)a2);
  }
}

// the key of sort pass `which` (0 minor, 1 position, 2 referenceId) of the row
// at each position of `order` (null: the rows as added, and idx gets 0, 1, ..)
extern "C" __global__ void __launch_bounds__(kThreads) agg_sort_key(Rows R, const uint64_t* minor, int which,
                                                                     const uint32_t* order, int64_t n, uint64_t* key,
                                                                     uint32_t* idx) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t r = order ? order[j] : (uint32_t)j;
    key[j] = which == 0 ? minor[r] : which == 1 ? key_position(R.position[r]) : key_reference(R.reference_id[r]);
    if (!order) idx[j] = (uint32_t)j;
  }
}

// flags[j]: bit 0 the sorted row j starts a group, bit 1 it goes on a group
// with another record-group code than the row before it
extern "C" __global__ void __launch_bounds__(kThreads) agg_heads(Rows R, const uint64_t* minor, const uint32_t* order,
                                                                  int64_t n, uint8_t* flags) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t r = order[j];
    uint8_t f = 1;
    if (j > 0) {
      const uint32_t p = order[j - 1];
      const bool head = minor[r] != minor[p] || R.position[r] != R.position[p] || R.reference_id[r] != R.reference_id[p];
      f = head ? 1 : (R.rg[r] != R.rg[p] ? 2 : 0);
    }
    flags[j] = f;
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) agg_names(const int32_t* name, const uint32_t* order, int64_t n,
                                                                  int32_t* out) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x)
    out[j] = name[order[j]];
}

// ---- the scans -----------------------------------------------------------

struct S1 {
  uint32_t head;   // a group starts somewhere in the span
  uint32_t heads;  // how many (not segmented: the group index)
  uint32_t cnt, soft, rev, chg;
  uint32_t bad;  // rows with a null that a fold of two or more rows throws on
  int64_t mn, mx;
};
struct Op1 {
  __device__ __forceinline__ static S1 identity() { return S1{0, 0, 0, 0, 0, 0, 0, INT64_MAX, INT64_MIN}; }
  __device__ __forceinline__ S1 operator()(const S1& a, const S1& b) const {
    if (b.head) return S1{1, a.heads + b.heads, b.cnt, b.soft, b.rev, b.chg, b.bad, b.mn, b.mx};
    return S1{a.head, a.heads + b.heads, a.cnt + b.cnt, a.soft + b.soft, a.rev + b.rev, a.chg + b.chg,
              a.bad + b.bad, a.mn < b.mn ? a.mn : b.mn, a.mx > b.mx ? a.mx : b.mx};
  }
  __device__ __forceinline__ static S1 up(const S1& v, int d) {
    return S1{(uint32_t)__shfl_up((int)v.head, d),       (uint32_t)__shfl_up((int)v.heads, d),
              (uint32_t)__shfl_up((int)v.cnt, d),        (uint32_t)__shfl_up((int)v.soft, d),
              (uint32_t)__shfl_up((int)v.rev, d),        (uint32_t)__shfl_up((int)v.chg, d),
              (uint32_t)__shfl_up((int)v.bad, d),
              (int64_t)__shfl_up((long long)v.mn, d),    (int64_t)__shfl_up((long long)v.mx, d)};
  }
};

// x -> x * A + B over Z / 2^32, for mapQuality and sangerQuality at once
struct S2 {
  uint32_t a, bm, bs;
};
struct Op2 {
  __device__ __forceinline__ static S2 identity() { return S2{1, 0, 0}; }
  __device__ __forceinline__ S2 operator()(const S2& x, const S2& y) const {
    return S2{x.a * y.a, x.bm * y.a + y.bm, x.bs * y.a + y.bs};
  }
  __device__ __forceinline__ static S2 up(const S2& v, int d) {
    return S2{(uint32_t)__shfl_up((int)v.a, d), (uint32_t)__shfl_up((int)v.bm, d), (uint32_t)__shfl_up((int)v.bs, d)};
  }
};

// inclusive scan over the NW * 64 threads of a workgroup, in thread order:
// across the lanes by shuffles, the wave totals through `lds` (NW entries);
// *total = the whole workgroup's.  Every thread calls it.
template <int NW, class T, class Op>
__device__ __forceinline__ T block_scan(T v, Op op, T* lds, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const T o = Op::up(v, d);
    if (lane >= d) v = op(o, v);
  }
  __syncthreads();  // (lds may still be read from the call before)
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  T pre = Op::identity(), all = Op::identity();
  for (int w = 0; w < NW; ++w) {
    const T x = lds[w];
    if (w < wave) pre = op(pre, x);
    all = op(all, x);
  }
  *total = all;
  return op(pre, v);
}

// the tile totals, in place, to their inclusive scan (one workgroup)
template <class T, class Op>
__device__ __forceinline__ void top_scan(T* agg, int64_t n_tiles, T* lds) {
  Op op;
  T carry = Op::identity();
  for (int64_t b = 0; b < n_tiles; b += kTopThreads) {
    const int64_t i = b + threadIdx.x;
    T total;
    T v = block_scan<kTopThreads / 64>(i < n_tiles ? agg[i] : Op::identity(), op, lds, &total);
    if (i < n_tiles) agg[i] = op(carry, v);
    carry = op(carry, total);
  }
}
extern "C" __global__ void __launch_bounds__(kTopThreads) agg_top1(S1* agg, int64_t n_tiles) {
  __shared__ S1 lds[kTopThreads / 64];
  top_scan<S1, Op1>(agg, n_tiles, lds);
}
extern "C" __global__ void __launch_bounds__(kTopThreads) agg_top2(S2* agg, int64_t n_tiles) {
  __shared__ S2 lds[kTopThreads / 64];
  top_scan<S2, Op2>(agg, n_tiles, lds);
}

struct Groups {
  uint32_t* offsets;  // [n_groups + 1] first sorted row of each group
  uint32_t *cnt, *soft, *rev, *chg, *bad, *m, *s;
  int64_t *mn, *mx;
};

struct ScanParams {
  Rows R;
  const uint32_t* order;
  const uint8_t* flags;
  int64_t n, n_tiles;
  S1* agg1;
  S2* agg2;
  uint2* row;  // per sorted row: C_{k-1} (the group's count before it), the group index
  Groups G;
  unsigned long long* err;
};

__device__ __forceinline__ S1 load1(const ScanParams& P, int64_t j, uint32_t r, uint32_t f) {
  return S1{f & 1u, f & 1u, (uint32_t)P.R.count[r], (uint32_t)P.R.soft[r], (uint32_t)P.R.rev[r], (f >> 1) & 1u,
            ((uint32_t)P.R.mask[r] & (kEveryRow | kDeepRow)) != (kEveryRow | kDeepRow) ? 1u : 0u, P.R.read_start[r],
            P.R.read_end[r]};
}

// scan 1, pass 1: the tile totals
extern "C" __global__ void __launch_bounds__(kThreads) agg_scan1_tiles(ScanParams P) {
  __shared__ S1 lds[kWaves];
  for (int64_t t = blockIdx.x; t < P.n_tiles; t += gridDim.x) {
    const int64_t j = t * kThreads + threadIdx.x;
    S1 e = Op1::identity();
    if (j < P.n) e = load1(P, j, P.order[j], P.flags[j]);
    S1 total;
    (void)block_scan<kWaves>(e, Op1(), lds, &total);
    if (threadIdx.x == 0) P.agg1[t] = total;
  }
}

// scan 1, pass 2 (agg1 scanned): every row's C_{k-1} and group index, the
// groups' plain folds at their last rows, the nulls that throw in groups of two
// or more; and the tile totals of scan 2
extern "C" __global__ void __launch_bounds__(kThreads) agg_scan1_rows(ScanParams P) {
  __shared__ S1 lds1[kWaves];
  __shared__ S2 lds2[kWaves];
  for (int64_t t = blockIdx.x; t < P.n_tiles; t += gridDim.x) {
    const int64_t j = t * kThreads + threadIdx.x;
    const bool live = j < P.n;
    uint32_t r = 0, f = 0;
    S1 e = Op1::identity();
    if (live) {
      r = P.order[j];
      f = P.flags[j];
      e = load1(P, j, r, f);
    }
    S1 total;
    S1 v = block_scan<kWaves>(e, Op1(), lds1, &total);
    if (t > 0) v = Op1()(P.agg1[t - 1], v);
    S2 x = Op2::identity();
    if (live) {
      const bool head = f & 1u;
      const bool last = j == P.n - 1 || (P.flags[j + 1] & 1u);
      const uint32_t before = v.cnt - e.cnt, g = v.heads - 1;
      P.row[j] = make_uint2(before, g);
      if (head) P.G.offsets[g] = (uint32_t)j;
      if (last) {
        P.G.cnt[g] = v.cnt;
        P.G.soft[g] = v.soft;
        P.G.rev[g] = v.rev;
        P.G.chg[g] = v.chg;
        P.G.bad[g] = v.bad;
        P.G.mn[g] = v.mn;
        P.G.mx[g] = v.mx;
      }
      if (!(head && last) && ((uint32_t)P.R.mask[r] & kDeepRow) != kDeepRow)
        atomicMin(P.err, ((unsigned long long)r << 8) | (unsigned long long)BQSR_ERR_NULL_FIELD);
      const uint32_t c = (uint32_t)P.R.count[r], mq = (uint32_t)P.R.mapq[r], sq = (uint32_t)P.R.sanger[r];
      x = head ? S2{0, mq, sq} : S2{before, mq * c, sq * c};
    }
    S2 total2;
    (void)block_scan<kWaves>(x, Op2(), lds2, &total2);
    if (threadIdx.x == 0) P.agg2[t] = total2;
  }
}

// scan 2, pass 2 (agg2 scanned): (M, S) at every group's last row
extern "C" __global__ void __launch_bounds__(kThreads) agg_scan2_rows(ScanParams P) {
  __shared__ S2 lds[kWaves];
  for (int64_t t = blockIdx.x; t < P.n_tiles; t += gridDim.x) {
    const int64_t j = t * kThreads + threadIdx.x;
    const bool live = j < P.n;
    S2 x = Op2::identity();
    uint2 rw = make_uint2(0, 0);
    bool last = false;
    if (live) {
      const uint32_t r = P.order[j], f = P.flags[j];
      rw = P.row[j];
      last = j == P.n - 1 || (P.flags[j + 1] & 1u);
      const uint32_t c = (uint32_t)P.R.count[r], mq = (uint32_t)P.R.mapq[r], sq = (uint32_t)P.R.sanger[r];
      x = (f & 1u) ? S2{0, mq, sq} : S2{rw.x, mq * c, sq * c};
    }
    S2 total;
    S2 v = block_scan<kWaves>(x, Op2(), lds, &total);
    if (t > 0) v = Op2()(P.agg2[t - 1], v);
    if (live && last) {  // (the map applied to anything: A = 0 since the group's head)
      P.G.m[rw.y] = v.bm;
      P.G.s[rw.y] = v.bs;
    }
  }
}

// ---- emit ----------------------------------------------------------------

enum : int { kVRoff = 0, kVRlen, kVRefBase, kVReadBase, kVSoft, kVRev, kVRstart, kVRend, kVUniform, kVWords };

struct Out {
  int32_t* reference_id;
  int64_t* position;
  int32_t *range_offset, *range_length;
  uint8_t *reference_base, *read_base;
  int32_t *sanger, *mapq, *soft, *rev, *count;
  int64_t *read_start, *read_end;
  uint32_t* first_row;
  uint64_t* v[kVWords];  // [ceil(n_groups / 64)]
};

struct EmitParams {
  Rows R;
  const uint32_t* order;
  Groups G;
  int64_t n_groups;
  Out O;
  unsigned long long* err;
};

// Java's int division: toward zero, Int.MinValue / -1 = Int.MinValue (b != 0)
__device__ __forceinline__ int32_t java_div(uint32_t a, uint32_t b) {
  if (b == 0xFFFFFFFFu) return (int32_t)(0u - a);
  return (int32_t)a / (int32_t)b;
}

extern "C" __global__ void __launch_bounds__(kThreads) agg_emit(EmitParams P) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t words = (P.n_groups + 63) >> 6;
  for (int64_t w = wave0; w < words; w += waves) {
    const int64_t g = (w << 6) + lane;
    const bool live = g < P.n_groups;
    uint32_t m = 0, r = 0, c = 0;
    bool uniform = false;
    if (live) {
      r = P.order[P.G.offsets[g]];
      m = P.R.mask[r];
      c = P.G.cnt[g];
      uniform = P.G.chg[g] == 0;
      // a division by zero, unless a null in the group has thrown before it
      const bool lone = P.G.offsets[g + 1] - P.G.offsets[g] == 1;
      const bool thrown = lone ? (m & kEveryRow) != kEveryRow : P.G.bad[g] != 0;
      if (c == 0 && !thrown) atomicMin(P.err, ((unsigned long long)r << 8) | (unsigned long long)BQSR_ERR_PILEUP);
    }
    auto has = [&](uint32_t k) -> bool { return live && ((m >> k) & 1u); };
    const uint64_t b0 = __builtin_amdgcn_ballot_w64(has(kRoff)), b1 = __builtin_amdgcn_ballot_w64(has(kRlen)),
                   b2 = __builtin_amdgcn_ballot_w64(has(kRefBase)), b3 = __builtin_amdgcn_ballot_w64(has(kReadBase)),
                   b4 = __builtin_amdgcn_ballot_w64(has(kSoft)), b5 = __builtin_amdgcn_ballot_w64(has(kRev)),
                   b6 = __builtin_amdgcn_ballot_w64(has(kRstart)), b7 = __builtin_amdgcn_ballot_w64(has(kRend)),
                   b8 = __builtin_amdgcn_ballot_w64(live && uniform);
    if (lane == 0) {
      P.O.v[kVRoff][w] = b0;
      P.O.v[kVRlen][w] = b1;
      P.O.v[kVRefBase][w] = b2;
      P.O.v[kVReadBase][w] = b3;
      P.O.v[kVSoft][w] = b4;
      P.O.v[kVRev][w] = b5;
      P.O.v[kVRstart][w] = b6;
      P.O.v[kVRend][w] = b7;
      P.O.v[kVUniform][w] = b8;
    }
    if (live) {
      P.O.reference_id[g] = P.R.reference_id[r];
      P.O.position[g] = P.R.position[r];
      P.O.range_offset[g] = has(kRoff) ? P.R.range_offset[r] : 0;
      P.O.range_length[g] = has(kRlen) ? P.R.range_length[r] : 0;
      P.O.reference_base[g] = has(kRefBase) ? P.R.reference_base[r] : 0;
      P.O.read_base[g] = has(kReadBase) ? P.R.read_base[r] : 0;
      P.O.sanger[g] = c ? java_div(P.G.s[g], c) : 0;
      P.O.mapq[g] = c ? java_div(P.G.m[g], c) : 0;
      P.O.soft[g] = has(kSoft) ? (int32_t)P.G.soft[g] : 0;
      P.O.rev[g] = has(kRev) ? (int32_t)P.G.rev[g] : 0;
      P.O.count[g] = (int32_t)c;
      P.O.read_start[g] = has(kRstart) ? P.G.mn[g] : 0;
      P.O.read_end[g] = has(kRend) ? P.G.mx[g] : 0;
      P.O.first_row[g] = r;
    }
  }
}

}  // namespace pagk

struct bqsr_pileup_agg {
  bqsr_context* ctx = nullptr;
  pagk::Rows R{};
  int64_t cap = 0, n = 0;
  // the last run's result
  bool ran = false;
  int64_t n_groups = 0;
  uint32_t* order = nullptr;
  uint32_t* offsets = nullptr;
  int32_t* names = nullptr;
  pagk::Out O{};
  std::vector<void*> result;
  unsigned long long* err = nullptr;  // the grouping error word, the six key statistics, the fold error word
  StageClock<5> clock;  // (AGG_MARKS below)
  void drop_result() {
    for (void* p : result) (void)hipFree(p);
    result.clear();
    ran = false;
    n_groups = 0;
    order = offsets = nullptr;
    names = nullptr;
  }
  ~bqsr_pileup_agg() {
    drop_result();
    for (void** p : columns())
      if (*p) (void)hipFree(*p);
    if (err) (void)hipFree(err);
  }
  std::array<void**, 17> columns() {
    return {(void**)&R.reference_id, (void**)&R.position,       (void**)&R.range_offset, (void**)&R.range_length,
            (void**)&R.reference_base, (void**)&R.read_base,    (void**)&R.sanger,       (void**)&R.mapq,
            (void**)&R.soft,         (void**)&R.rev,            (void**)&R.count,        (void**)&R.read_start,
            (void**)&R.read_end,     (void**)&R.sample,         (void**)&R.rg,           (void**)&R.name,
            (void**)&R.mask};
  }
};

namespace {

constexpr size_t kAggWidth[17] = {4, 8, 4, 4, 1, 1, 4, 4, 4, 4, 4, 8, 8, 4, 4, 4, 2};
constexpr int64_t kAggMaxRows = 2147483647LL;

// the stages of the calling thread's last run (aggregate_pileups.KERNELS): stage k lies between marks k and k + 1
enum { AGG_KEYS, AGG_SORT, AGG_SCANS, AGG_EMIT, AGG_STAGES };
// the clock's marks: each between two ends one stage and starts the next
enum { AGG_KEYS_0, AGG_SORT_0, AGG_SCANS_0, AGG_EMIT_0, AGG_EMIT_1, AGG_MARKS };
static_assert(AGG_MARKS == 5, "bqsr_pileup_agg::clock holds AGG_MARKS marks");
thread_local double g_agg_ms[AGG_STAGES] = {0.0, 0.0, 0.0, 0.0};

// room for `more` rows after the handle's: the columns grow by doubling, the rows kept
bqsr_status agg_reserve(bqsr_pileup_agg* h, int64_t more, hipStream_t s, const char* who) {
  if (more > kAggMaxRows - h->n)
    return fail(BQSR_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 - 1 rows in one aggregation");
  h->drop_result();
  const int64_t need = h->n + more;
  if (need <= h->cap) return BQSR_OK;
  const int64_t cap = std::min<int64_t>(kAggMaxRows, std::max<int64_t>({need, 2 * h->cap, 1024}));
  auto cols = h->columns();
  for (int k = 0; k < 17; ++k) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, (size_t)cap * kAggWidth[k]));
    if (h->n) HIP_TRY(hipMemcpyAsync(p, *cols[k], (size_t)h->n * kAggWidth[k], hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (*cols[k]) (void)hipFree(*cols[k]);
    *cols[k] = p;
  }
  h->cap = cap;
  return BQSR_OK;
}

const char* agg_what(int status) {
  switch (status) {
    case BQSR_ERR_NULL_FIELD:
      return "a null referenceId or position, or for the fold a null mapQuality, sangerQuality or countAtPosition or, "
             "in a group of two or more rows, a null numSoftClipped, numReverseStrand, readStart or readEnd (the "
             "reference throws a NullPointerException)";
    case BQSR_ERR_PILEUP:
      return "the group this row starts has a countAtPosition sum of 0 (the reference's division throws an "
             "ArithmeticException)";
    default:
      return "a sample code outside [0, 2^22 - 2]";
  }
}

bqsr_status agg_error(unsigned long long ew, const char* who) {
  const int status = (int)(ew & 0xFF);
  const int64_t row = (int64_t)(ew >> 8);
  return fail((bqsr_status)status, std::string(who) + ": row " + std::to_string(row) + ": " + agg_what(status), row);
}

// the rows of the last prepare on a parse, emitted into the handle
bqsr_status agg_add_reads(bqsr_context* ctx, bqsr_pileup_agg* h, PileupState& A, const PileupView& V,
                          const int32_t* ref_id, const int32_t* sample_code, const int32_t* rg_code, int64_t name_base,
                          hipStream_t s, const char* who) {
  if (name_base < 0 || name_base + A.n > 2147483647LL)
    return fail(BQSR_ERR_UNSUPPORTED, std::string(who) + ": read ordinals beyond 2^31 - 1");
  if (!A.prepared) return fail(BQSR_ERR_INVALID_ARG, std::string(who) + " before its prepare call");
  const int64_t m = A.n_rows;
  if (m == 0) return ok();
  bqsr_status e;
  if ((e = agg_reserve(h, m, s, who)) != BQSR_OK) return e;
  SortTmp T;
  int32_t *read, *d_sample, *d_rg;
  uint64_t* words;
  const size_t W = (size_t)((m + 63) / 64);
  if ((e = sam_alloc(T.v, &read, (size_t)m)) || (e = sam_alloc(T.v, &words, 4 * W)) ||
      (e = sam_alloc(T.v, &d_sample, (size_t)A.n)) || (e = sam_alloc(T.v, &d_rg, (size_t)A.n)))
    return e;
  HIP_TRY(hipMemcpyAsync(d_sample, sample_code, (size_t)A.n * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_rg, rg_code, (size_t)A.n * 4, hipMemcpyHostToDevice, s));
  const int64_t b = h->n;
  pilk::Cols C{};
  C.read = read;
  C.position = h->R.position + b;
  C.range_offset = h->R.range_offset + b;
  C.range_length = h->R.range_length + b;
  C.reference_base = h->R.reference_base + b;
  C.read_base = h->R.read_base + b;
  C.sanger = h->R.sanger + b;
  C.mapq = h->R.mapq + b;
  C.soft = h->R.soft + b;
  C.rev = h->R.rev + b;
  C.read_start = h->R.read_start + b;
  C.read_end = h->R.read_end + b;
  C.v_range = words;
  C.v_reference_base = words + W;
  C.v_read_base = words + 2 * W;
  C.v_mapq = words + 3 * W;
  pilk::EmitParams P{V.R, A.X, A.rs, A.r0, A.n, m, C};
  const int64_t groups = (m + 63) / 64;
  JOB_TRY(launch(pilk::pileup_emit, pileup_grid(ctx, (groups + pilk::kWaves - 1) / pilk::kWaves), pilk::kThreads, s,
                 P));
  pagk::PackReads Q{h->R, b, m, A.r0, name_base, read, words, words + W, words + 2 * W, words + 3 * W, ref_id, d_sample, d_rg};
  JOB_TRY(launch(pagk::agg_pack_reads, pileup_grid(ctx, (m + pagk::kThreads - 1) / pagk::kThreads), pagk::kThreads, s,
                 Q));
  HIP_TRY(hipStreamSynchronize(s));  // (the temporaries go)
  h->n += m;
  return ok();
}

}  // namespace

extern "C" {

bqsr_status bqsr_pileup_agg_create(bqsr_context* ctx, bqsr_pileup_agg** out) {
  if (!ctx || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_pileup_agg_create: bad arguments");
  *out = nullptr;
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<bqsr_pileup_agg> h(new (std::nothrow) bqsr_pileup_agg);
  if (!h) return fail(BQSR_ERR_DEVICE, "bqsr_pileup_agg_create: out of memory");
  h->ctx = ctx;
  HIP_TRY(hipMalloc((void**)&h->err, 8 * 8));
  *out = h.release();
  return ok();
}

void bqsr_pileup_agg_destroy(bqsr_pileup_agg* agg) { delete agg; }

bqsr_status bqsr_pileup_agg_add_host(bqsr_pileup_agg* h, const bqsr_pileup_agg_rows* rows, void* stream) {
  if (!h || !rows || rows->n_rows < 0) return fail(BQSR_ERR_INVALID_ARG, "bqsr_pileup_agg_add_host: bad arguments");
  if (!rows->rg_code && rows->n_rows)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_pileup_agg_add_host: no record-group codes");
  const int64_t m = rows->n_rows;
  if (m == 0) return ok();
  HIP_TRY(hipSetDevice(h->ctx->device));
  hipStream_t s = S(stream);
  bqsr_status e;
  if ((e = agg_reserve(h, m, s, "bqsr_pileup_agg_add_host")) != BQSR_OK) return e;
  const void* src[16] = {rows->reference_id,   rows->position,           rows->range_offset, rows->range_length,
                         rows->reference_base, rows->read_base,          rows->sanger_quality, rows->map_quality,
                         rows->num_soft_clipped, rows->num_reverse_strand, rows->count_at_position, rows->read_start,
                         rows->read_end,       rows->sample_code,        rows->rg_code,
                         rows->name_code};
  const uint8_t* valid[pagk::kCols] = {rows->reference_id_valid,   rows->position_valid,
                                       rows->range_offset_valid,   rows->range_length_valid,
                                       rows->reference_base_valid, rows->read_base_valid,
                                       rows->sanger_quality_valid, rows->map_quality_valid,
                                       rows->num_soft_clipped_valid, rows->num_reverse_strand_valid,
                                       rows->count_at_position_valid, rows->read_start_valid,
                                       rows->read_end_valid,       rows->sample_code_valid};
  auto cols = h->columns();
  SortTmp T;
  pagk::PackHost P{};
  P.R = h->R;
  P.base = h->n;
  P.n = m;
  const size_t vb = (size_t)((m + 7) / 8);
  P.implicit_names = rows->name_code ? 0 : 1;
  for (int k = 0; k < 16; ++k) {
    uint8_t* dst = (uint8_t*)*cols[k] + (size_t)h->n * kAggWidth[k];
    if (src[k]) HIP_TRY(hipMemcpyAsync(dst, src[k], (size_t)m * kAggWidth[k], hipMemcpyHostToDevice, s));
    else HIP_TRY(hipMemsetAsync(dst, 0, (size_t)m * kAggWidth[k], s));  // a column not given: every value null
    if (k >= (int)pagk::kCols) continue;
    if (src[k]) P.present |= 1u << k;
    if (src[k] && valid[k]) {
      uint8_t* dv;
      if ((e = sam_alloc(T.v, &dv, vb)) != BQSR_OK) return e;
      HIP_TRY(hipMemcpyAsync(dv, valid[k], vb, hipMemcpyHostToDevice, s));
      P.bm[k] = dv;
    }
  }
  JOB_TRY(launch(pagk::agg_pack_host, pileup_grid(h->ctx, (m + pagk::kThreads - 1) / pagk::kThreads), pagk::kThreads, s,
                 P));
  HIP_TRY(hipStreamSynchronize(s));  // (the staged bitmaps go, the caller's buffers are free)
  h->n += m;
  return ok();
}

bqsr_status bqsr_sam_pileup_agg_add(bqsr_context* ctx, bqsr_sam* sm, bqsr_pileup_agg* agg, const int32_t* sample_code,
                                    const int32_t* rg_code, int64_t name_base, void* stream) {
  if (!ctx || !sm || !agg || !sample_code || !rg_code)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_pileup_agg_add: bad arguments");
  if (!sm->pileup) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_pileup_agg_add before bqsr_sam_pileup_prepare");
  HIP_TRY(hipSetDevice(ctx->device));
  return agg_add_reads(ctx, agg, *job_state<PileupState>(sm->pileup), pileup_view(sm), sm->sq_id, sample_code, rg_code,
                       name_base, S(stream), "bqsr_sam_pileup_agg_add");
}

bqsr_status bqsr_arrow_pileup_agg_add(bqsr_context* ctx, bqsr_arrow* a, bqsr_pileup_agg* agg,
                                      const int32_t* sample_code, const int32_t* rg_code, int64_t name_base,
                                      void* stream) {
  if (!ctx || !a || !agg || !sample_code || !rg_code)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_pileup_agg_add: bad arguments");
  if (!a->pileup) return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_pileup_agg_add before bqsr_arrow_pileup_prepare");
  HIP_TRY(hipSetDevice(ctx->device));
  PileupState& A = *job_state<PileupState>(a->pileup);
  return agg_add_reads(ctx, agg, A, pileup_view(a, A), a->sq, sample_code, rg_code, name_base, S(stream),
                       "bqsr_arrow_pileup_agg_add");
}

bqsr_status bqsr_pileup_agg_run(bqsr_pileup_agg* h, void* stream, bqsr_pileup_agg_sizes* out) {
  if (!h || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_pileup_agg_run: bad arguments");
  const char* who = "aggregate_pileups";
  bqsr_context* ctx = h->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  h->drop_result();
  out->n_rows = h->n;
  out->n_groups = 0;
  out->bitmap_words = 0;
  for (double& v : g_agg_ms) v = 0.0;
  const int64_t n = h->n;
  if (n == 0) {
    h->ran = true;
    return ok();
  }
  const size_t N = (size_t)n;
  const int64_t n_tiles = (n + pagk::kThreads - 1) / pagk::kThreads;
  const unsigned grid = pileup_grid(ctx, n_tiles);
  bqsr_status e;
  SortTmp T;
  uint64_t *minor, *key_a, *key_b;
  uint32_t *idx_a, *idx_b;
  uint8_t* flags;
  pagk::S1* agg1;
  pagk::S2* agg2;
  if ((e = sam_alloc(T.v, &minor, N)) || (e = sam_alloc(T.v, &key_a, N)) || (e = sam_alloc(T.v, &key_b, N)) ||
      (e = sam_alloc(T.v, &idx_a, N)) || (e = sam_alloc(h->result, &idx_b, N)) || (e = sam_alloc(T.v, &flags, N)) ||
      (e = sam_alloc(T.v, &agg1, (size_t)n_tiles)) || (e = sam_alloc(T.v, &agg2, (size_t)n_tiles)))
    return e;
  // keys
  unsigned long long init[8] = {~0ull, 0, 0, 0, ~0ull, ~0ull, ~0ull, ~0ull}, st[8];
  HIP_TRY(hipMemcpyAsync(h->err, init, sizeof init, hipMemcpyHostToDevice, s));
  HIP_TRY(h->clock.mark(AGG_KEYS_0, s));
  JOB_TRY(launch(pagk::agg_keys, grid, pagk::kThreads, s, pagk::KeysParams{h->R, n, minor, h->err, h->err + 7,
                 h->err + 1}));
  HIP_TRY(h->clock.mark(AGG_SORT_0, s));
  HIP_TRY(hipMemcpyAsync(st, h->err, sizeof st, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (st[0] != ~0ull) {
    h->drop_result();
    return agg_error(st[0], who);
  }
  // sort: LSD over the three keys, each over the bits in which its keys differ.
  // idx_b (kept with the result) ends up holding the order.
  uint32_t *cur = nullptr, *src = idx_a, *dst = idx_b;
  int passes = 0;
  for (int which = 0; which < 3; ++which)
    if (which == 0 || (st[1 + which] ^ st[4 + which])) ++passes;
  if (passes == 2) std::swap(src, dst);  // (an even number of passes ends where it began)
  size_t tb = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, key_a, key_b, src, dst, N, 0, 64, s));
  uint8_t* temp;
  if ((e = sam_alloc(T.v, &temp, tb)) != BQSR_OK) return e;
  for (int which = 0; which < 3; ++which) {
    const int bits = bits_of((uint64_t)(st[1 + which] ^ st[4 + which]));
    if (which && !bits) continue;
    JOB_TRY(launch(pagk::agg_sort_key, grid, pagk::kThreads, s, h->R, minor, which, cur, n, key_a, src));
    size_t tb2 = tb;
    HIP_TRY(rocprim::radix_sort_pairs(temp, tb2, key_a, key_b, src, dst, N, 0, std::max(1, bits), s));
    cur = dst;
    std::swap(src, dst);
  }
  const uint32_t* order = cur;  // == idx_b
  HIP_TRY(h->clock.mark(AGG_SCANS_0, s));
  // heads, scan 1 pass 1, the number of groups
  JOB_TRY(launch(pagk::agg_heads, grid, pagk::kThreads, s, h->R, minor, order, n, flags));
  pagk::ScanParams P{};
  P.R = h->R;
  P.order = order;
  P.flags = flags;
  P.n = n;
  P.n_tiles = n_tiles;
  P.agg1 = agg1;
  P.agg2 = agg2;
  P.row = (uint2*)key_a;
  P.err = h->err + 7;
  JOB_TRY(launch(pagk::agg_scan1_tiles, grid, pagk::kThreads, s, P));
  JOB_TRY(launch(pagk::agg_top1, 1, pagk::kTopThreads, s, agg1, n_tiles));
  pagk::S1 last;
  HIP_TRY(hipMemcpyAsync(&last, agg1 + (n_tiles - 1), sizeof last, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int64_t G = (int64_t)last.heads;
  const size_t NG = (size_t)G, W = (size_t)((G + 63) / 64);
  pagk::Groups& Gr = P.G;
  if ((e = sam_alloc(h->result, &Gr.offsets, NG + 1)) || (e = sam_alloc(T.v, &Gr.cnt, NG)) ||
      (e = sam_alloc(T.v, &Gr.soft, NG)) || (e = sam_alloc(T.v, &Gr.rev, NG)) || (e = sam_alloc(T.v, &Gr.chg, NG)) ||
      (e = sam_alloc(T.v, &Gr.bad, NG)) ||
      (e = sam_alloc(T.v, &Gr.m, NG)) || (e = sam_alloc(T.v, &Gr.s, NG)) || (e = sam_alloc(T.v, &Gr.mn, NG)) ||
      (e = sam_alloc(T.v, &Gr.mx, NG)))
    return e;
  pagk::Out& O = h->O;
  std::vector<void*>& keep = h->result;
  if ((e = sam_alloc(keep, &O.reference_id, NG)) || (e = sam_alloc(keep, &O.position, NG)) ||
      (e = sam_alloc(keep, &O.range_offset, NG)) || (e = sam_alloc(keep, &O.range_length, NG)) ||
      (e = sam_alloc(keep, &O.reference_base, NG)) || (e = sam_alloc(keep, &O.read_base, NG)) ||
      (e = sam_alloc(keep, &O.sanger, NG)) || (e = sam_alloc(keep, &O.mapq, NG)) || (e = sam_alloc(keep, &O.soft, NG)) ||
      (e = sam_alloc(keep, &O.rev, NG)) || (e = sam_alloc(keep, &O.count, NG)) ||
      (e = sam_alloc(keep, &O.read_start, NG)) || (e = sam_alloc(keep, &O.read_end, NG)) ||
      (e = sam_alloc(keep, &O.first_row, NG)))
    return e;
  for (int k = 0; k < pagk::kVWords; ++k)
    if ((e = sam_alloc(keep, &O.v[k], W)) != BQSR_OK) return e;
  const uint32_t n32 = (uint32_t)n;
  HIP_TRY(hipMemcpyAsync(Gr.offsets + G, &n32, 4, hipMemcpyHostToDevice, s));
  JOB_TRY(launch(pagk::agg_scan1_rows, grid, pagk::kThreads, s, P));
  JOB_TRY(launch(pagk::agg_top2, 1, pagk::kTopThreads, s, agg2, n_tiles));
  JOB_TRY(launch(pagk::agg_scan2_rows, grid, pagk::kThreads, s, P));
  HIP_TRY(h->clock.mark(AGG_EMIT_0, s));
  const int64_t words = (G + 63) / 64;
  JOB_TRY(launch(pagk::agg_emit, pileup_grid(ctx, (words + pagk::kWaves - 1) / pagk::kWaves), pagk::kThreads, s,
                 pagk::EmitParams{h->R, order, Gr, G, O, h->err + 7}));
  HIP_TRY(h->clock.mark(AGG_EMIT_1, s));
  int32_t* names;
  if ((e = sam_alloc(keep, &names, N)) != BQSR_OK) return e;
  JOB_TRY(launch(pagk::agg_names, grid, pagk::kThreads, s, h->R.name, order, n, names));
  unsigned long long ew = ~0ull;
  HIP_TRY(hipMemcpyAsync(&ew, h->err + 7, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  h->clock.add(g_agg_ms[AGG_KEYS], AGG_KEYS_0, AGG_SORT_0);
  h->clock.add(g_agg_ms[AGG_SORT], AGG_SORT_0, AGG_SCANS_0);
  h->clock.add(g_agg_ms[AGG_SCANS], AGG_SCANS_0, AGG_EMIT_0);
  h->clock.add(g_agg_ms[AGG_EMIT], AGG_EMIT_0, AGG_EMIT_1);
  if (ew != ~0ull) {
    h->drop_result();
    return agg_error(ew, who);
  }
  h->order = idx_b;
  h->offsets = Gr.offsets;
  h->names = names;
  h->n_groups = G;
  h->ran = true;
  out->n_groups = G;
  out->bitmap_words = words;
  return ok();
}

bqsr_status bqsr_pileup_agg_fetch(bqsr_pileup_agg* h, const bqsr_pileup_agg_host* dst, void* stream) {
  if (!h || !dst) return fail(BQSR_ERR_INVALID_ARG, "bqsr_pileup_agg_fetch: bad arguments");
  if (!h->ran) return fail(BQSR_ERR_INVALID_ARG, "bqsr_pileup_agg_fetch before a bqsr_pileup_agg_run that succeeded");
  if (h->n == 0) {
    if (dst->offsets) dst->offsets[0] = 0;
    return ok();
  }
  HIP_TRY(hipSetDevice(h->ctx->device));
  hipStream_t s = S(stream);
  const size_t g = (size_t)h->n_groups, W = (g + 63) / 64;
  const pagk::Out& O = h->O;
  auto cp = [&](void* d, const void* src, size_t bytes) -> hipError_t {
    if (!d || !bytes) return hipSuccess;
    return hipMemcpyAsync(d, src, bytes, hipMemcpyDeviceToHost, s);
  };
  hipError_t e = cp(dst->reference_id, O.reference_id, g * 4);
  if (e == hipSuccess) e = cp(dst->position, O.position, g * 8);
  if (e == hipSuccess) e = cp(dst->range_offset, O.range_offset, g * 4);
  if (e == hipSuccess) e = cp(dst->range_length, O.range_length, g * 4);
  if (e == hipSuccess) e = cp(dst->reference_base, O.reference_base, g);
  if (e == hipSuccess) e = cp(dst->read_base, O.read_base, g);
  if (e == hipSuccess) e = cp(dst->sanger_quality, O.sanger, g * 4);
  if (e == hipSuccess) e = cp(dst->map_quality, O.mapq, g * 4);
  if (e == hipSuccess) e = cp(dst->num_soft_clipped, O.soft, g * 4);
  if (e == hipSuccess) e = cp(dst->num_reverse_strand, O.rev, g * 4);
  if (e == hipSuccess) e = cp(dst->count_at_position, O.count, g * 4);
  if (e == hipSuccess) e = cp(dst->read_start, O.read_start, g * 8);
  if (e == hipSuccess) e = cp(dst->read_end, O.read_end, g * 8);
  if (e == hipSuccess) e = cp(dst->first_row, O.first_row, g * 4);
  if (e == hipSuccess) e = cp(dst->offsets, h->offsets, (g + 1) * 4);
  if (e == hipSuccess) e = cp(dst->order, h->order, (size_t)h->n * 4);
  if (e == hipSuccess) e = cp(dst->names, h->names, (size_t)h->n * 4);
  uint64_t* const words[pagk::kVWords] = {dst->range_offset_valid,   dst->range_length_valid,
                                          dst->reference_base_valid, dst->read_base_valid,
                                          dst->num_soft_clipped_valid, dst->num_reverse_strand_valid,
                                          dst->read_start_valid,     dst->read_end_valid, dst->uniform_rg};
  for (int k = 0; k < pagk::kVWords; ++k)
    if (e == hipSuccess) e = cp(words[k], O.v[k], W * 8);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(BQSR_ERR_DEVICE, std::string("bqsr_pileup_agg_fetch: ") + hipGetErrorString(e));
  return ok();
}

bqsr_status bqsr_pileup_agg_kernel_times(double* keys_ms, double* sort_ms, double* scans_ms, double* emit_ms) {
  if (keys_ms) *keys_ms = g_agg_ms[AGG_KEYS];
  if (sort_ms) *sort_ms = g_agg_ms[AGG_SORT];
  if (scans_ms) *scans_ms = g_agg_ms[AGG_SCANS];
  if (emit_ms) *emit_ms = g_agg_ms[AGG_EMIT];
  return BQSR_OK;
}

}  // extern "C"
