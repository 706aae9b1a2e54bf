// `adam flagstat` on the device (include/adam_sam.h: bqsr_sam_flagstat,
// bqsr_flagstat_arrow): adamFlagStat (core/rdd/FlagStat.scala:21-116), the
// eighteen counters of FlagStatMetrics kept once for the reads that passed the
// vendor quality checks and once for those that failed them.
//
// One reduction core, two front ends.  The core works on 64-bit masks of a
// group of 64 consecutive reads (bit l = read i0 + l): the nine booleans,
// "referenceId != mateReferenceId" (Scala's != on boxed Integers: null equals
// null, null differs from a value), "mapq >= 5" and "mapq is null".  Every
// counter is the popcount of an AND / ANDN expression of those masks, split
// by the failed mask.  A lane owns one group at a time, so a wavefront counts
// up to 64 groups with one pass of popcounts; the 36 sums stay in the lanes'
// registers over the grid-stride loop, are summed over the wave by shuffles
// and over the workgroup's waves through LDS, and the workgroup issues one
// 64-bit atomicAdd per non-zero counter.  Integer sums: the result does not
// depend on the launch order.  A read with mateMappedToDiffChromosome and a
// null mapq makes the reference unbox null (FlagStat.scala:100): the smallest
// such read index is kept by atomicMin and the call returns
// BQSR_ERR_NULL_FIELD.
//
//   flagstat_sam    a lane per read of a parse: FLAG (raw_flag, with the flags
//       column's duplicateRead bit), referenceId (sq_id), and MAPQ / RNEXT
//       found in the read's line and turned into mapq / mateReferenceId by
//       adam_fields.h -- the code the ADAM columns use; ballots make the
//       group's masks, which go to the next free lane
//   flagstat_arrow  Arrow buffers, a wavefront per tile of 64 groups: a bitmap
//       word is a mask as it stands (AND its validity word: a null boolean
//       reads as false), so lane l loads the words of group l, coalesced; the
//       three int32 columns go lane per read, four groups a pass so that
//       twelve loads per lane are in flight, and their ballots go to the
//       group's lane
//
// Included by bqsr_capi.cpp after sam_sort.hip (sam_alloc and SortTmp come from
// the files before it).

#include "adam_fields.h"

namespace fstk {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCounters = 18;
constexpr int kWords = 2 * kCounters + 1;  // passed, failed, the first NULL_FIELD read
constexpr int kFirstNull = 2 * kCounters;
constexpr int kUnroll = 4;                  // groups per pass of flagstat_arrow's int columns
// the booleans in the order of bqsr_flagstat_chunk
enum { kPaired, kProper, kMapped, kMateMapped, kFirst, kSecond, kPrimary, kDup, kFailed, kBools };

// the masks of the group a lane owns (all zero: no group)
struct Masks {
  uint64_t b[kBools];
  uint64_t ne;     // referenceId != mateReferenceId (null-aware)
  uint64_t q5;     // mapq >= 5
  uint64_t qnull;  // mapq is null
  uint64_t live;   // the group's reads
};

__device__ __forceinline__ void masks_clear(Masks& m) {
#pragma unroll
  for (int k = 0; k < kBools; ++k) m.b[k] = 0;
  m.ne = m.q5 = m.qnull = m.live = 0;
}

// per lane, 32 bits: a lane adds at most 64 per group it owns, so a counter
// would need 2^26 groups on one lane -- 2^38 reads on one wavefront -- to wrap
struct Acc {
  uint32_t c[2 * kCounters];
  unsigned long long first_null;
};

__device__ __forceinline__ void acc_init(Acc& a) {
#pragma unroll
  for (int k = 0; k < 2 * kCounters; ++k) a.c[k] = 0;
  a.first_null = ~0ull;
}

// the counters of this lane's group (FlagStat.scala:29-46, 88-101); every
// mask is clipped to the group's live reads; i0 = the global index of bit 0
__device__ __forceinline__ void acc_lane(Acc& a, const Masks& m, int64_t i0) {
  const uint64_t P = m.b[kPaired], M = m.b[kMapped], MM = m.b[kMateMapped], D = m.b[kDup], PR = m.b[kPrimary];
  const uint64_t dp = D & PR, ds = D & ~PR;
  const uint64_t both = M & MM, only = M & ~MM;
  const uint64_t diff = P & both & m.ne;
  const uint64_t x[kCounters] = {m.live,
                                 dp, dp & both, dp & only, dp & m.ne,
                                 ds, ds & both, ds & only, ds & m.ne,
                                 M, P, P & m.b[kFirst], P & m.b[kSecond], P & m.b[kProper],
                                 P & both, P & only, diff, diff & m.q5};
  const uint64_t F = m.b[kFailed];
#pragma unroll
  for (int k = 0; k < kCounters; ++k) {
    a.c[k] += (uint32_t)__popcll(x[k] & ~F);
    a.c[kCounters + k] += (uint32_t)__popcll(x[k] & F);
  }
  const uint64_t bad = diff & m.qnull;
  if (bad) {
    const unsigned long long r = (unsigned long long)i0 + (unsigned long long)__builtin_ctzll(bad);
    a.first_null = r < a.first_null ? r : a.first_null;
  }
}

// lanes -> wave by shuffles, the workgroup's waves through LDS, then one
// atomic per non-zero counter
__device__ __forceinline__ void acc_finish(const Acc& a, unsigned long long* out) {
  __shared__ unsigned long long sh[kWaves][2 * kCounters];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long first = a.first_null;
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(first, d);
    first = o < first ? o : first;
  }
#pragma unroll
  for (int k = 0; k < 2 * kCounters; ++k) {
    unsigned long long v = a.c[k];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) sh[wave][k] = v;
  }
  if (lane == 0 && first != ~0ull) atomicMin(&out[kFirstNull], first);
  __syncthreads();
  if (threadIdx.x < 2 * kCounters) {
    unsigned long long v = 0;
    for (int w = 0; w < kWaves; ++w) v += sh[w][threadIdx.x];
    if (v) atomicAdd(&out[threadIdx.x], v);
  }
}

__device__ __forceinline__ uint64_t live_mask(int64_t n, int64_t i0) {
  const int64_t c = n - i0;
  return c >= 64 ? ~0ull : (c <= 0 ? 0ull : ((1ull << c) - 1ull));
}

extern "C" __global__ void __launch_bounds__(kThreads) flagstat_sam(const uint8_t* __restrict__ text,
                                                                    const uint64_t* __restrict__ line_span,
                                                                    const uint32_t* __restrict__ raw_flag,
                                                                    const uint32_t* __restrict__ flags,
                                                                    const int32_t* __restrict__ sq_id,
                                                                    samk::NameTable sq_tab, int64_t n, int64_t base,
                                                                    unsigned long long* out) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  Acc a;
  acc_init(a);
  Masks m;  // lane u: the u-th group this wave met since the last acc_lane
  masks_clear(m);
  int64_t my_i0 = 0;
  int u = 0;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < n; i0 += stride) {
    const int64_t i = i0 + lane;
    const bool live = i < n;
    uint32_t f = 0;
    int32_t sq = -1, msq = -1;
    bool has_mapq = false;
    int64_t mapq = 255;
    if (live) {
      f = adamk::flag_with_dup(raw_flag[i], flags[i]);
      sq = sq_id[i];
      // MAPQ is field 5, RNEXT field 7 of the line (the parse saw 11 fields)
      const int64_t e = (int64_t)line_span[2 * i + 1];
      int64_t p = (int64_t)line_span[2 * i], a4 = 0, b4 = 0, a6 = 0, b6 = 0;
      for (int k = 0; k < 7; ++k) {
        const int64_t fa = p;
        while (p < e && text[p] != '\t') ++p;
        if (k == 4) a4 = fa, b4 = p;
        if (k == 6) a6 = fa, b6 = p;
        if (p < e) ++p;
      }
      has_mapq = adamk::mapq_field(text, a4, b4, sq, &mapq);
      msq = adamk::rnext_id(sq_tab, text, a6, b6, sq);
    }
    const int kBit[kBools] = {0, 1, 2, 3, 6, 7, 8, 10, 9};  // flag_bit's numbering, in kPaired .. kFailed order
    const bool mine = lane == u;
#pragma unroll
    for (int k = 0; k < kBools; ++k) {
      const uint64_t w = __builtin_amdgcn_ballot_w64(live && adamk::flag_bit(f, kBit[k]));
      if (mine) m.b[k] = w;
    }
    const uint64_t ne = __builtin_amdgcn_ballot_w64(live && sq != msq);  // null is -1 on both sides
    const uint64_t q5 = __builtin_amdgcn_ballot_w64(live && has_mapq && mapq >= 5);
    const uint64_t qnull = __builtin_amdgcn_ballot_w64(live && !has_mapq);
    if (mine) {
      m.ne = ne;
      m.q5 = q5;
      m.qnull = qnull;
      m.live = live_mask(n, i0);
      my_i0 = base + i0;
    }
    if (++u == 64) {
      acc_lane(a, m, my_i0);
      masks_clear(m);
      u = 0;
    }
  }
  if (u) acc_lane(a, m, my_i0);  // (the lanes from u on hold no group)
  acc_finish(a, out);
}

// One Arrow chunk on the device.  Bitmaps as 64-bit words (the buffers are
// padded to whole words; bits at and beyond n are masked here).  A null
// boolean column is all false, a null validity all valid, a null int column
// all null.
struct ArrowChunk {
  const uint64_t* b[kBools];
  const uint64_t* bv[kBools];
  const int32_t* iv[3];    // referenceId, mateReferenceId, mapq
  const uint64_t* ivv[3];
  int64_t n, base;
};

// bit `lane` of lane u's 64-bit word w (u uniform)
__device__ __forceinline__ bool lane_bit(uint64_t w, int u, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)w, u);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(w >> 32), u);
  return ((lane < 32 ? lo >> lane : hi >> (lane - 32)) & 1u) != 0;
}

extern "C" __global__ void __launch_bounds__(kThreads) flagstat_arrow(ArrowChunk C, unsigned long long* out) {
  const int lane = threadIdx.x & 63;
  const int64_t n_groups = (C.n + 63) >> 6;
  const int64_t n_tiles = (n_groups + 63) >> 6;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  Acc a;
  acc_init(a);
  for (int64_t t = wave0; t < n_tiles; t += waves) {
    // this lane's group: its bitmap words
    const int64_t g = (t << 6) + lane;
    const bool in = g < n_groups;
    Masks m;
    m.live = in ? live_mask(C.n, g << 6) : 0ull;
#pragma unroll
    for (int k = 0; k < kBools; ++k)
      m.b[k] = in && C.b[k] ? C.b[k][g] & (C.bv[k] ? C.bv[k][g] : ~0ull) & m.live : 0ull;
    uint64_t vw[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) vw[c] = in && C.iv[c] ? (C.ivv[c] ? C.ivv[c][g] & m.live : m.live) : 0ull;
    m.qnull = ~vw[2] & m.live;
    m.ne = m.q5 = 0;
    // the tile's groups one after the other, a lane per read
    const int ng = (int)min((int64_t)64, n_groups - (t << 6));
    for (int u0 = 0; u0 < ng; u0 += kUnroll) {
      int32_t v[kUnroll][3];
#pragma unroll
      for (int uu = 0; uu < kUnroll; ++uu) {
        const int64_t i = (((t << 6) + u0 + uu) << 6) + lane;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[uu][c] = C.iv[c] && i < C.n ? C.iv[c][i] : 0;
      }
#pragma unroll
      for (int uu = 0; uu < kUnroll; ++uu) {
        const int u = u0 + uu;
        if (u >= ng) break;  // (uniform)
        const bool rv = lane_bit(vw[0], u, lane), mv = lane_bit(vw[1], u, lane), qv = lane_bit(vw[2], u, lane);
        const uint64_t ne = __builtin_amdgcn_ballot_w64(rv != mv || (rv && v[uu][0] != v[uu][1]));
        const uint64_t q5 = __builtin_amdgcn_ballot_w64(qv && v[uu][2] >= 5);
        if (lane == u) {
          m.ne = ne;
          m.q5 = q5;
        }
      }
    }
    acc_lane(a, m, C.base + (g << 6));
  }
  acc_finish(a, out);
}

}  // namespace fstk

namespace {

// the context's counter block, held for one call (the call ends in a
// synchronise): allocated on first use, freed with the context
struct FlagstatDev {
  std::unique_lock<std::mutex> lock;
  unsigned long long* d = nullptr;
};

bqsr_status flagstat_begin(bqsr_context* ctx, FlagstatDev& F, hipStream_t s) {
  F.lock = std::unique_lock<std::mutex>(ctx->flagstat_mu);
  if (!ctx->d_flagstat) HIP_TRY(hipMalloc((void**)&ctx->d_flagstat, fstk::kWords * 8));
  F.d = ctx->d_flagstat;
  HIP_TRY(hipMemsetAsync(F.d, 0, fstk::kFirstNull * 8, s));
  HIP_TRY(hipMemsetAsync(F.d + fstk::kFirstNull, 0xFF, 8, s));
  return BQSR_OK;
}

// the counters to the host; NULL_FIELD (and no counts) when a read was caught
bqsr_status flagstat_end(FlagstatDev& F, hipStream_t s, const char* who, bqsr_flagstat* out) {
  unsigned long long h[fstk::kWords];
  HIP_TRY(hipMemcpyAsync(h, F.d, sizeof h, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h[fstk::kFirstNull] != ~0ull) {
    char buf[240];
    snprintf(buf, sizeof buf,
             "%s: read %llu has its mate mapped to a different chromosome and a null mapq (the reference's "
             "getMapq >= 5 throws a NullPointerException)",
             who, h[fstk::kFirstNull]);
    return fail(BQSR_ERR_NULL_FIELD, buf, (int64_t)h[fstk::kFirstNull]);
  }
  for (int k = 0; k < fstk::kCounters; ++k) {
    out->passed.c[k] = (int64_t)h[k];
    out->failed.c[k] = (int64_t)h[fstk::kCounters + k];
  }
  return ok();
}

// workgroups for `units` wavefronts' worth of work (flagstat_sam: groups,
// flagstat_arrow: tiles of 64 groups), at most per_cu of them per CU -- or
// at most BQSR_TUNE_FLAGSTAT_GRID in all
unsigned flagstat_grid(const bqsr_context* ctx, int64_t units, int per_cu) {
  const int64_t cap = ctx->tune_flagstat_grid > 0 ? ctx->tune_flagstat_grid : (int64_t)ctx->n_cu * per_cu;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((units + fstk::kWaves - 1) / fstk::kWaves, cap));
}

}  // namespace

extern "C" {

bqsr_status bqsr_sam_flagstat(bqsr_context* ctx, const bqsr_sam* sm, void* stream, bqsr_flagstat* out) {
  if (!ctx || !sm || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_flagstat: bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  memset(out, 0, sizeof *out);
  const int64_t n = sm->n_reads;
  if (n == 0) return ok();
  FlagstatDev F;
  bqsr_status e;
  if ((e = flagstat_begin(ctx, F, s)) != BQSR_OK) return e;
  JOB_TRY(launch(fstk::flagstat_sam, flagstat_grid(ctx, (n + 63) / 64, 8), fstk::kThreads, s, sm->d_text, sm->line_span,
                 sm->raw_flag, sm->flags, sm->sq_id, sm->sq_tab, n, (int64_t)0, F.d));
  return flagstat_end(F, s, "flagstat", out);
}

bqsr_status bqsr_flagstat_arrow(bqsr_context* ctx, const bqsr_flagstat_chunk* chunks, int32_t n_chunks, void* stream,
                                bqsr_flagstat* out) {
  if (!ctx || !out || n_chunks < 0 || (n_chunks && !chunks))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_flagstat_arrow: bad arguments");
  int64_t max_n = 0;
  for (int32_t c = 0; c < n_chunks; ++c) {
    if (chunks[c].n_reads < 0) return fail(BQSR_ERR_INVALID_ARG, "bqsr_flagstat_arrow: negative chunk length");
    max_n = std::max(max_n, chunks[c].n_reads);
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  memset(out, 0, sizeof *out);
  if (max_n == 0) return ok();
  FlagstatDev F;
  bqsr_status e;
  if ((e = flagstat_begin(ctx, F, s)) != BQSR_OK) return e;
  // one staging area, sized for the largest chunk: 21 bitmaps of whole
  // 64-bit words, then the three int32 columns
  const size_t W = (size_t)((max_n + 63) / 64);
  const int kMaps = 2 * fstk::kBools + 3;
  SortTmp T;
  uint64_t* maps;
  int32_t* ints;
  if ((e = sam_alloc(T.v, &maps, W * kMaps)) || (e = sam_alloc(T.v, &ints, (size_t)max_n * 3))) return e;
  int64_t r0 = 0;
  for (int32_t c = 0; c < n_chunks; ++c) {
    const bqsr_flagstat_chunk& H = chunks[c];
    const int64_t m = H.n_reads;
    if (m == 0) continue;
    const size_t vb = (size_t)(m + 7) / 8;  // the bytes the caller's bitmaps hold
    int slot = 0;
    auto bitmap = [&](const uint8_t* src, const uint64_t** dst) -> hipError_t {
      *dst = nullptr;
      if (!src) return hipSuccess;
      uint64_t* d = maps + (size_t)slot++ * W;
      *dst = d;
      return hipMemcpyAsync(d, src, vb, hipMemcpyHostToDevice, s);
    };
    fstk::ArrowChunk C{};
    C.n = m;
    C.base = r0;
    for (int k = 0; k < fstk::kBools; ++k) {
      HIP_TRY(bitmap(H.bools[k], &C.b[k]));
      HIP_TRY(bitmap(H.bools[k] ? H.bools_validity[k] : nullptr, &C.bv[k]));
    }
    const int32_t* iv[3] = {H.reference_id, H.mate_reference_id, H.mapq};
    const uint8_t* ivv[3] = {H.reference_id_validity, H.mate_reference_id_validity, H.mapq_validity};
    for (int k = 0; k < 3; ++k) {
      if (iv[k]) {
        int32_t* d = ints + (size_t)k * (size_t)max_n;
        HIP_TRY(hipMemcpyAsync(d, iv[k], (size_t)m * 4, hipMemcpyHostToDevice, s));
        C.iv[k] = d;
      }
      HIP_TRY(bitmap(iv[k] ? ivv[k] : nullptr, &C.ivv[k]));
    }
    const int64_t groups = (m + 63) / 64;
    JOB_TRY(launch(fstk::flagstat_arrow, flagstat_grid(ctx, (groups + 63) / 64, 4), fstk::kThreads, s, C, F.d));
    r0 += m;
  }
  return flagstat_end(F, s, "flagstat", out);
}

/* measurement only: the Arrow-form kernel alone over device buffers
 * (tools/bench_adam.py --flagstat times it with events): every pointer of
 * `chunk` is device memory, bitmaps padded to whole 64-bit words; `counters`
 * = 37 device words (36 sums, then the first NULL_FIELD read), accumulated
 * into.  Nothing about the buffers is checked. */
bqsr_status bqsr_flagstat_arrow_device(bqsr_context* ctx, const bqsr_flagstat_chunk* chunk, void* counters,
                                       void* stream) {
  if (!ctx || !chunk || !counters || chunk->n_reads < 0)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_flagstat_arrow_device: bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  fstk::ArrowChunk C{};
  C.n = chunk->n_reads;
  for (int k = 0; k < fstk::kBools; ++k) {
    C.b[k] = (const uint64_t*)chunk->bools[k];
    C.bv[k] = chunk->bools[k] ? (const uint64_t*)chunk->bools_validity[k] : nullptr;
  }
  C.iv[0] = chunk->reference_id;
  C.iv[1] = chunk->mate_reference_id;
  C.iv[2] = chunk->mapq;
  C.ivv[0] = chunk->reference_id ? (const uint64_t*)chunk->reference_id_validity : nullptr;
  C.ivv[1] = chunk->mate_reference_id ? (const uint64_t*)chunk->mate_reference_id_validity : nullptr;
  C.ivv[2] = chunk->mapq ? (const uint64_t*)chunk->mapq_validity : nullptr;
  if (C.n == 0) return ok();
  const int64_t groups = (C.n + 63) / 64;
  JOB_TRY(launch(fstk::flagstat_arrow, flagstat_grid(ctx, (groups + 63) / 64, 4), fstk::kThreads, S(stream), C,
                 (unsigned long long*)counters));
  return ok();
}

}  // extern "C"
