// Indel realignment targets on the device (include/adam_sam.h:
// bqsr_sam_realign_targets_*, bqsr_arrow_realign_targets_*):
// RealignmentTargetFinder.findTargets (core/algorithms/realignmenttarget/
// RealignmentTargetFinder.scala:54-101) over IndelRealignmentTarget.apply,
// merge and TargetOrdering.overlap (IndelRealignmentTarget.scala:41-101,
// 251-437) over the ADAMPileup rows of Reads2PileupProcessor (pileup.hip).
//
// One job over all reads of a parse layout (a SAM / BAM parse or the layout
// bqsr_arrow_load builds), which stays resident.  Nothing but the results
// leaves the device, except the candidates' (start, end) pairs for the fold:
//
//   rt_count      a lane per read: pileup.hip's walk_read (the same row
//       counts, statuses, prefixes and readEnd), plus the refusal of a read
//       with rows and a start below 0 (positions are key bits); the lowest
//       throwing read by atomicMin, the largest readEnd by atomicMax.
//   (scan)        row counts -> first row of each read.
//   rt_emit       a lane per ROW, coalesced stores: key = position; payload =
//       class (match, mismatch, insert or clip, delete) | read ordinal |
//       sangerQuality (match, mismatch) or the CIGAR element's index in the
//       read (delete: the indel range is start + refpre .. + length - 1).
//       The read by binary search over the row prefix, the element over the
//       element prefix, the MD entry over the read's list.  A mismatch is
//       readBase != referenceBase, not "the MD names a base there".
//   (sort)        stable rocprim::radix_sort_pairs over the position bits in
//       use: referenceId is not part of the key, as in the reference.
//   rt_heads, (scan), (reduce_by_key)   rod heads, rod ids, and per rod the
//       two Java Int quality sums, carried as the two wrapping 32-bit halves
//       of one 64-bit word.
//   rt_evflag, (scan), rt_events   a row is an event when it is an indel row,
//       or a mismatch of a rod with matchQuality == 0 or (double)
//       mismatchQuality / (double) matchQuality >= 0.15 (IEEE double); events
//       (rod | kind, a, b, readStart, readEnd - 1) are written in rod order.
//   (reduce_by_key)   per rod with events -- a candidate -- the hull of its
//       events' read ranges; the unique keys are the candidates, compacted.
//   rt_candkeys, (sort), rt_gather   candidates ascending by (start,
//       position): a stable radix sort by start of candidates that are in
//       position order already.
//   the fold      joinTargets is the one serial step: it runs in C++ on the
//       host over the downloaded (start, end) pairs, with
//       TargetOrdering.overlap's four clauses as written; the target id of
//       every candidate and the "two or more candidates" flag of every target
//       go back up.  The targets' own ranges are the fold's state.
//   rt_rod2t, rt_retarget, (merge_sort)   events keyed by (target, kind, a, b,
//       readStart, readEnd).
//   (reduce_by_key)   exact duplicates collapse everywhere; indel events of a
//       target merged from two or more candidates collapse by (target,
//       indelRange) into the hull of their read ranges, which is what the
//       chain of merge calls with its RangeAccumulator leaves.  A target from
//       a single rod never went through merge and keeps them apart.
//   rt_isindel, (scan), rt_write, rt_offsets   the sorted survivors are the
//       result arrays in their declared order; offsets per target by binary
//       search.
//
// HBM per row as built: 16 B key, 16 B payload (both double-buffered for the
// sort; the spare halves then hold the heads, rod ids, quality words and event
// flags) and 4 B event offset: 36 B, plus rocprim's workspace; 80 B per event.

namespace rtk {

constexpr int kThreads = 256;
enum { kMatch = 0, kMismatch = 1, kInsert = 2, kDelete = 3 };

// g: rod << 1 | kind until the fold, then target << 1 | kind (kind 0: indel,
// 1: SNP); a..b the indel range or the SNP site twice; rs..re the read range
struct Ev {
  int64_t g, a, b, rs, re;
};

struct QSum {  // two Java Ints side by side, each wrapping on its own
  __host__ __device__ uint64_t operator()(uint64_t x, uint64_t y) const {
    const uint32_t lo = (uint32_t)x + (uint32_t)y, hi = (uint32_t)(x >> 32) + (uint32_t)(y >> 32);
    return ((uint64_t)hi << 32) | lo;
  }
};

struct Hull {  // the left element with the hull of both read ranges
  __host__ __device__ Ev operator()(const Ev& x, const Ev& y) const {
    return Ev{x.g, x.a, x.b, x.rs < y.rs ? x.rs : y.rs, x.re > y.re ? x.re : y.re};
  }
};

struct RodOf {
  __host__ __device__ int64_t operator()(const Ev& e) const { return e.g >> 1; }
};

struct EvLess {
  __host__ __device__ bool operator()(const Ev& x, const Ev& y) const {
    if (x.g != y.g) return x.g < y.g;
    if (x.a != y.a) return x.a < y.a;
    if (x.b != y.b) return x.b < y.b;
    if (x.rs != y.rs) return x.rs < y.rs;
    return x.re < y.re;
  }
};

// one element of a target's sets: an exact duplicate, or an indel range of a
// target that went through merge
struct EvSame {
  const uint8_t* multi;  // per target: folded from two or more candidates
  __host__ __device__ bool operator()(const Ev& x, const Ev& y) const {
    if (x.g != y.g || x.a != y.a || x.b != y.b) return false;
    if (!(x.g & 1) && multi[x.g >> 1]) return true;
    return x.rs == y.rs && x.re == y.re;
  }
};

struct CountParams {
  pilk::CountParams P;
  unsigned long long* maxend;  // atomicMax of readEnd over the reads with rows
};

extern "C" __global__ void __launch_bounds__(kThreads) rt_count(CountParams C) {
  const pilk::Reads& R = C.P.R;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < C.P.n; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t rows;
    int st = pilk::walk_read(C.P, i, i, &rows);
    // positions are key bits: none below 0; a delete's element index takes 31 bits
    if (!st && rows && (R.start[i] < 0 || R.cig_off[i + 1] - R.cig_off[i] > 2147483647ull)) st = BQSR_ERR_UNSUPPORTED;
    C.P.X.cnt[i] = st ? 0 : rows;
    if (st) atomicMin(C.P.err, ((unsigned long long)i << 8) | (unsigned long long)st);
    else if (rows) atomicMax(C.maxend, (unsigned long long)C.P.X.rend[i]);
  }
}

struct EmitParams {
  pilk::Reads R;
  pilk::Scratch X;
  const uint64_t* rs;  // [n + 1] first row of each read
  int64_t n, n_rows;
  uint64_t* key;  // position
  uint64_t* val;  // class | read << 2 | (quality byte or element index) << 33
};

extern "C" __global__ void __launch_bounds__(kThreads) rt_emit(EmitParams P) {
  const pilk::Reads& R = P.R;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < P.n_rows; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = pilk::last_le(P.rs, 0, P.n - 1, (uint64_t)g);
    const uint32_t w = (uint32_t)((uint64_t)g - P.rs[i]);  // position in the walk (the sets do not care for row order)
    const uint64_t c0 = R.cig_off[i];
    int64_t ea = 0, eb = (int64_t)(R.cig_off[i + 1] - c0) - 1;
    while (ea < eb) {  // the last element with rowpre <= w
      const int64_t m = (ea + eb + 1) >> 1;
      if (P.X.rowpre[c0 + m] <= w) ea = m;
      else eb = m - 1;
    }
    const uint32_t e = R.cig[c0 + ea], op = bqsr::cig_op(e);
    const uint32_t k = w - P.X.rowpre[c0 + ea];
    const bool is_m = op == BQSR_CIGAR_M, is_d = op == BQSR_CIGAR_D;
    const int64_t rp = (int64_t)P.X.readpre[c0 + ea] + (is_d ? 0 : k);
    const int64_t ro = P.X.refpre[c0 + ea] + ((is_m || is_d) ? k : 0);
    uint32_t cls = is_d ? kDelete : kInsert;  // I and S rows: rangeOffset set, readBase set
    uint64_t extra = is_d ? (uint64_t)ea : 0;
    if (is_m) {
      const uint32_t* ent = P.X.mdent + R.md_off[i];
      int64_t a = 0, b = P.X.md_n[i];
      while (a < b) {  // first entry with offset >= ro
        const int64_t m = (a + b) >> 1;
        if ((int64_t)(ent[m] >> 6) < ro) a = m + 1;
        else b = m;
      }
      const int read_base = pilk::base_index(R.seq[R.seq_off[i] + rp]);
      const bool hit = a < (int64_t)P.X.md_n[i] && (int64_t)(ent[a] >> 6) == ro;
      cls = hit && (int)(ent[a] & 31u) != read_base ? kMismatch : kMatch;
      extra = (uint8_t)(R.qual[R.qual_off[i] + rp] - 33);
    }
    P.key[g] = (uint64_t)(R.start[i] + ro);
    P.val[g] = (uint64_t)cls | ((uint64_t)i << 2) | (extra << 33);
  }
}

// a rod starts where the position changes; q = matchQuality | mismatchQuality << 32 of the row
extern "C" __global__ void __launch_bounds__(kThreads) rt_heads(const uint64_t* key, const uint64_t* val, int64_t m,
                                                               uint32_t* head, uint64_t* q) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    head[j] = j == 0 || key[j - 1] != key[j];
    const uint64_t v = val[j];
    const uint32_t cls = (uint32_t)(v & 3);
    const uint32_t sanger = (uint32_t)(int32_t)(int8_t)(uint8_t)(v >> 33);  // .toByte, widened
    q[j] = cls == kMatch ? (uint64_t)sanger : cls == kMismatch ? (uint64_t)sanger << 32 : 0;
  }
}

// IndelRealignmentTarget.apply's test on the rod's two Int sums
__device__ __forceinline__ bool keeps_snps(uint64_t q) {
  const int32_t match_q = (int32_t)(uint32_t)q, mismatch_q = (int32_t)(uint32_t)(q >> 32);
  return match_q == 0 || (double)mismatch_q / (double)match_q >= 0.15;
}

extern "C" __global__ void __launch_bounds__(kThreads) rt_evflag(const uint64_t* val, const uint32_t* rod1,
                                                                const uint64_t* rodq, int64_t m, uint32_t* isev) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t cls = (uint32_t)(val[j] & 3);
    isev[j] = cls >= kInsert || (cls == kMismatch && keeps_snps(rodq[rod1[j] - 1]));
    if (j == 0) isev[m] = 0;
  }
}

struct EventParams {
  pilk::Reads R;
  pilk::Scratch X;
  const uint64_t* key;
  const uint64_t* val;
  const uint32_t* rod1;
  const uint32_t* isev;
  const uint32_t* evoff;
  int64_t m;
  Ev* ev;
};

extern "C" __global__ void __launch_bounds__(kThreads) rt_events(EventParams P) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < P.m; j += (int64_t)gridDim.x * blockDim.x) {
    if (!P.isev[j]) continue;
    const uint64_t v = P.val[j];
    const uint32_t cls = (uint32_t)(v & 3);
    const int64_t i = (int64_t)((v >> 2) & 0x7FFFFFFFull);
    const int64_t pos = (int64_t)P.key[j];
    int64_t a = pos, b = pos;
    if (cls == kDelete) {  // position - rangeOffset .. + rangeLength - 1
      const uint64_t c = P.R.cig_off[i] + (v >> 33);
      a = P.R.start[i] + P.X.refpre[c];
      b = a + (int64_t)bqsr::cig_len(P.R.cig[c]) - 1;
    }
    P.ev[P.evoff[j]] = Ev{((int64_t)(P.rod1[j] - 1) << 1) | (cls == kMismatch ? 1 : 0), a, b, P.R.start[i],
                          P.X.rend[i] - 1};
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) rt_candkeys(const Ev* hull, int64_t nc, uint64_t* ckey,
                                                                  uint32_t* cval) {
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x) {
    ckey[c] = (uint64_t)hull[c].rs;
    cval[c] = (uint32_t)c;
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) rt_gather(const Ev* hull, const uint32_t* cval, int64_t nc,
                                                                int64_t* cend) {
  for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < nc; s += (int64_t)gridDim.x * blockDim.x)
    cend[s] = hull[cval[s]].re;
}

extern "C" __global__ void __launch_bounds__(kThreads) rt_rod2t(const int64_t* candrod, const uint32_t* cval,
                                                               const uint32_t* tid, int64_t nc, uint32_t* rod2t) {
  for (int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; s < nc; s += (int64_t)gridDim.x * blockDim.x)
    rod2t[candrod[cval[s]]] = tid[s];
}

extern "C" __global__ void __launch_bounds__(kThreads) rt_retarget(Ev* ev, int64_t n, const uint32_t* rod2t) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = ev[j].g;
    ev[j].g = ((int64_t)rod2t[g >> 1] << 1) | (g & 1);
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) rt_isindel(const Ev* out, int64_t n, uint32_t* isi) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    isi[e] = !(out[e].g & 1);
    if (e == 0) isi[n] = 0;
  }
}

struct Result {
  int64_t *indel_start, *indel_end, *indel_read_start, *indel_read_end;  // [n_out] each (n_indels in use)
  int64_t *snp_site, *snp_read_start, *snp_read_end;                     // [n_out] each (n_snps in use)
  int64_t *indel_offset, *snp_offset;                                    // [n_targets + 1]
};

// the survivors are sorted by (target, kind, ...): the indel ones, in order, are the indel arrays
extern "C" __global__ void __launch_bounds__(kThreads) rt_write(const Ev* out, const uint32_t* islot, int64_t n,
                                                               Result D) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const Ev v = out[e];
    const int64_t o = islot[e];
    if (!(v.g & 1)) {
      D.indel_start[o] = v.a;
      D.indel_end[o] = v.b;
      D.indel_read_start[o] = v.rs;
      D.indel_read_end[o] = v.re;
    } else {
      D.snp_site[e - o] = v.a;
      D.snp_read_start[e - o] = v.rs;
      D.snp_read_end[e - o] = v.re;
    }
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) rt_offsets(const Ev* out, const uint32_t* islot, int64_t n,
                                                                 int64_t n_targets, Result D) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t <= n_targets; t += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = 0, b = n;
    while (a < b) {  // the first survivor of target t or a later one
      const int64_t m = (a + b) >> 1;
      if (out[m].g < (t << 1)) a = m + 1;
      else b = m;
    }
    D.indel_offset[t] = islot[a];
    D.snp_offset[t] = a - (int64_t)islot[a];
  }
}

}  // namespace rtk

namespace {

struct RtState {
  DevBuf rowpre, readpre, refpre, mdent, cnt, rs, md_n, rend, small, key_a, key_b, val_a, val_b, evoff, rodq, ev_a, ev_b,
      candrod, hull, ckey_a, ckey_b, cval_a, cval_b, cend, tid, multi, rod2t, isi, islot, res, temp;
  rtk::Result D{};
  std::vector<int64_t> t_start, t_end;
  bqsr_realign_targets_sizes sizes{0, 0, 0, 0, 0, 0};
  bool prepared = false;
  StageClock<8> clock;
};

// the stages of the calling thread's last prepare (realignment_targets.KERNELS; the fold is timed on the host),
// and the clock's marks: count's end starts emit, emit's end sort, sort's end rods, rods' end candidates
enum { RT_COUNT, RT_EMIT, RT_SORT, RT_RODS, RT_CANDIDATES, RT_FOLD_HOST, RT_SETS, RT_STAGES };
enum { RT_COUNT_0, RT_EMIT_0, RT_SORT_0, RT_RODS_0, RT_CANDIDATES_0, RT_CANDIDATES_1, RT_SETS_0, RT_SETS_1 };
thread_local double g_realign_ms[RT_STAGES] = {0, 0, 0, 0, 0, 0, 0};

// joinTargets over singleton sets, left to right over the candidates in their
// declared order: the running last target a = (as, ae), the next candidate b
void rt_fold(const std::vector<uint64_t>& start, const std::vector<int64_t>& end, std::vector<uint32_t>& tid,
             std::vector<int64_t>& t_start, std::vector<int64_t>& t_end, std::vector<uint8_t>& multi) {
  t_start.clear();
  t_end.clear();
  multi.clear();
  for (size_t s = 0; s < start.size(); ++s) {
    const int64_t bs = (int64_t)start[s], be = end[s];
    if (!t_start.empty()) {
      const int64_t as = t_start.back(), ae = t_end.back();
      // TargetOrdering.overlap(a, b), as written
      const bool overlap = (as >= bs && as <= be) || (ae >= bs && ae <= bs) || (as >= bs && ae <= be) ||
                           (bs >= as && be <= ae);
      if (overlap) {  // a.merge(b)
        t_start.back() = std::min(as, bs);
        t_end.back() = std::max(ae, be);
        multi.back() = 1;
        tid[s] = (uint32_t)(t_start.size() - 1);
        continue;
      }
    }
    t_start.push_back(bs);
    t_end.push_back(be);
    multi.push_back(0);
    tid[s] = (uint32_t)(t_start.size() - 1);
  }
}

bqsr_status rt_prepare(bqsr_context* ctx, RtState& A, const PileupView& V, hipStream_t s,
                       bqsr_realign_targets_sizes* out) {
  using namespace rtk;
  A.prepared = false;
  A.sizes = bqsr_realign_targets_sizes{V.n_reads, 0, 0, 0, 0, 0};
  A.t_start.clear();
  A.t_end.clear();
  *out = A.sizes;
  for (double& t : g_realign_ms) t = 0.0;
  const int64_t n = V.n_reads;
  if (n > (int64_t)INT32_MAX)
    return fail(BQSR_ERR_UNSUPPORTED, "realignment_targets: more than 2^31 - 1 reads in one job");
  auto done = [&]() {
    *out = A.sizes;
    A.prepared = true;
    return ok();
  };
  if (n == 0) return done();
  // emit, sort and rods, read after a synchronize that follows the mark at rods' end
  auto upto_rods = [&]() {
    A.clock.add(g_realign_ms[RT_EMIT], RT_EMIT_0, RT_SORT_0);
    A.clock.add(g_realign_ms[RT_SORT], RT_SORT_0, RT_RODS_0);
    A.clock.add(g_realign_ms[RT_RODS], RT_RODS_0, RT_CANDIDATES_0);
  };
  bqsr_status e;
  auto need = [](DevBuf& b, auto** p, size_t count, const char* what) {
    return dev_need(b, p, count, "realignment_targets", what);
  };
  auto prim = [&](auto&& call) { return dev_prim(A.temp, "realignment_targets", call); };
  auto grid = [&](int64_t items) { return pileup_job_grid(ctx, items, kThreads); };
  // ---- count ----
  pilk::Scratch X{};
  uint64_t* rs;
  unsigned long long* small;  // the error word, the largest readEnd
  const size_t nc = (size_t)V.cig_ops, nm = (size_t)V.md_bytes, N = (size_t)n;
  if ((e = need(A.rowpre, &X.rowpre, nc, "CIGAR elements")) || (e = need(A.readpre, &X.readpre, nc, "CIGAR elements")) ||
      (e = need(A.refpre, &X.refpre, nc, "CIGAR elements")) || (e = need(A.mdent, &X.mdent, nm, "MD entries")) ||
      (e = need(A.cnt, &X.cnt, N + 1, "reads")) || (e = need(A.rs, &rs, N + 1, "reads")) ||
      (e = need(A.md_n, &X.md_n, N, "reads")) || (e = need(A.rend, &X.rend, N, "reads")) ||
      (e = need(A.small, &small, 2, "status words")))
    return e;
  HIP_TRY(hipMemsetAsync(small, 0xFF, 8, s));
  HIP_TRY(hipMemsetAsync(small + 1, 0, 8, s));
  HIP_TRY(hipMemsetAsync(X.cnt + n, 0, 8, s));
  CountParams C{pilk::CountParams{V.R, X, 0, n, small}, small + 1};
  HIP_TRY(A.clock.mark(RT_COUNT_0, s));
  JOB_TRY(launch(rt_count, grid(n), kThreads, s, C));
  HIP_TRY(A.clock.mark(RT_EMIT_0, s));
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::exclusive_scan(t, b, X.cnt, rs, (uint64_t)0, N + 1, rocprim::plus<uint64_t>(), s);
       })))
    return e;
  unsigned long long st2[2] = {~0ull, 0};
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(st2, small, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&total, rs + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  A.clock.add(g_realign_ms[RT_COUNT], RT_COUNT_0, RT_EMIT_0);
  if (st2[0] != ~0ull) {
    const int status = (int)(st2[0] & 0xFF);
    const int64_t read = (int64_t)(st2[0] >> 8);
    return fail((bqsr_status)status, "realignment_targets: read " + std::to_string(read) + ": " +
                (status == BQSR_ERR_UNSUPPORTED
                     ? "beyond the device path's limits (pileups of a read that starts below 0, a mismatch or deleted "
                       "base 2^26 or more positions after the read's start, or 2^31 or more rows, read bases or CIGAR "
                       "elements in one read)"
                     : pileup_what(status)), read);
  }
  if (total > (uint64_t)INT32_MAX)
    return fail(BQSR_ERR_UNSUPPORTED, "realignment_targets: more than 2^31 - 1 pileup rows in one job");
  const int64_t m = (int64_t)total;
  A.sizes.n_rows = m;
  if (m == 0) return done();
  const int pos_bits = std::max(1, bits_of((uint64_t)st2[1]));
  // ---- emit, sort ----
  const size_t M = (size_t)m;
  uint64_t *key_a, *key_b, *val_a, *val_b;
  if ((e = need(A.key_a, &key_a, M + 2, "pileup rows")) || (e = need(A.key_b, &key_b, M, "pileup rows")) ||
      (e = need(A.val_a, &val_a, M + 2, "pileup rows")) || (e = need(A.val_b, &val_b, M, "pileup rows")))
    return e;
  EmitParams E{V.R, X, rs, n, m, key_a, val_a};
  JOB_TRY(launch(rt_emit, grid(m), kThreads, s, E));
  HIP_TRY(A.clock.mark(RT_SORT_0, s));
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::radix_sort_pairs(t, b, key_a, key_b, val_a, val_b, M, 0, (unsigned)pos_bits, s);
       })))
    return e;
  HIP_TRY(A.clock.mark(RT_RODS_0, s));
  // ---- rods (the sort's spare halves hold the per-row words) ----
  uint64_t* q = key_a;                         // [M]
  uint32_t* head = (uint32_t*)val_a;           // [M + 2]; later the event flags
  uint32_t* rod1 = (uint32_t*)val_a + (M + 2);  // [M + 2]
  uint32_t* evoff;
  if ((e = need(A.evoff, &evoff, M + 1, "pileup rows"))) return e;
  JOB_TRY(launch(rt_heads, grid(m), kThreads, s, key_b, val_b, m, head, q));
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::inclusive_scan(t, b, head, rod1, M, rocprim::plus<uint32_t>(), s);
       })))
    return e;
  uint32_t n_rods32 = 0;
  HIP_TRY(hipMemcpyAsync(&n_rods32, rod1 + (m - 1), 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const size_t NR = n_rods32;
  uint64_t* rodq;
  if ((e = need(A.rodq, &rodq, NR + 1, "rods"))) return e;
  // (head is free: the unique keys go there, the count after the sums)
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::reduce_by_key(t, b, rod1, q, M, head, rodq, rodq + NR, QSum(), rocprim::equal_to<uint32_t>(), s);
       })))
    return e;
  uint32_t* isev = head;
  JOB_TRY(launch(rt_evflag, grid(m), kThreads, s, val_b, rod1, rodq, m, isev));
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::exclusive_scan(t, b, isev, evoff, (uint32_t)0, M + 1, rocprim::plus<uint32_t>(), s);
       })))
    return e;
  uint32_t n_ev32 = 0;
  HIP_TRY(hipMemcpyAsync(&n_ev32, evoff + m, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int64_t n_ev = n_ev32;
  const size_t NE = (size_t)n_ev;
  if (n_ev == 0) {
    HIP_TRY(A.clock.mark(RT_CANDIDATES_0, s));
    HIP_TRY(hipStreamSynchronize(s));
    upto_rods();
    return done();
  }
  Ev *ev_a, *ev_b, *hull;
  int64_t* candrod;
  if ((e = need(A.ev_a, &ev_a, NE, "events")) || (e = need(A.ev_b, &ev_b, NE, "events")) ||
      (e = need(A.hull, &hull, NE, "events")) || (e = need(A.candrod, &candrod, NE + 1, "events")))
    return e;
  EventParams EP{V.R, X, key_b, val_b, rod1, isev, evoff, m, ev_a};
  JOB_TRY(launch(rt_events, grid(m), kThreads, s, EP));
  HIP_TRY(A.clock.mark(RT_CANDIDATES_0, s));
  // ---- candidates: the rods with events, their hulls, ascending by (start, position) ----
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::reduce_by_key(t, b, rocprim::make_transform_iterator((const Ev*)ev_a, RodOf()), (const Ev*)ev_a,
                                       NE, candrod, hull, candrod + NE, Hull(), rocprim::equal_to<int64_t>(), s);
       })))
    return e;
  int64_t n_cand = 0;
  HIP_TRY(hipMemcpyAsync(&n_cand, candrod + NE, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const size_t NC = (size_t)n_cand;
  uint64_t *ckey_a, *ckey_b;
  uint32_t *cval_a, *cval_b, *tid, *rod2t;
  int64_t* cend;
  uint8_t* multi;
  if ((e = need(A.ckey_a, &ckey_a, NC, "candidates")) || (e = need(A.ckey_b, &ckey_b, NC, "candidates")) ||
      (e = need(A.cval_a, &cval_a, NC, "candidates")) || (e = need(A.cval_b, &cval_b, NC, "candidates")) ||
      (e = need(A.cend, &cend, NC, "candidates")) || (e = need(A.tid, &tid, NC, "candidates")) ||
      (e = need(A.multi, &multi, NC, "candidates")) || (e = need(A.rod2t, &rod2t, NR, "rods")))
    return e;
  JOB_TRY(launch(rt_candkeys, grid(n_cand), kThreads, s, hull, n_cand, ckey_a, cval_a));
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::radix_sort_pairs(t, b, ckey_a, ckey_b, cval_a, cval_b, NC, 0, (unsigned)pos_bits, s);
       })))
    return e;
  JOB_TRY(launch(rt_gather, grid(n_cand), kThreads, s, hull, cval_b, n_cand, cend));
  HIP_TRY(A.clock.mark(RT_CANDIDATES_1, s));
  std::vector<uint64_t> h_start(NC);
  std::vector<int64_t> h_end(NC);
  std::vector<uint32_t> h_tid(NC);
  std::vector<uint8_t> h_multi;
  HIP_TRY(hipMemcpyAsync(h_start.data(), ckey_b, NC * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(h_end.data(), cend, NC * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // ---- the fold ----
  const auto f0 = std::chrono::steady_clock::now();
  rt_fold(h_start, h_end, h_tid, A.t_start, A.t_end, h_multi);
  g_realign_ms[RT_FOLD_HOST] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - f0).count();
  const int64_t n_t = (int64_t)A.t_start.size();
  HIP_TRY(hipMemcpyAsync(tid, h_tid.data(), NC * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(multi, h_multi.data(), (size_t)n_t, hipMemcpyHostToDevice, s));
  // ---- the sets of every target ----
  HIP_TRY(A.clock.mark(RT_SETS_0, s));
  JOB_TRY(launch(rt_rod2t, grid(n_cand), kThreads, s, candrod, cval_b, tid, n_cand, rod2t));
  JOB_TRY(launch(rt_retarget, grid(n_ev), kThreads, s, ev_a, n_ev, rod2t));
  if ((e = prim([&](void* t, size_t& b) { return rocprim::merge_sort(t, b, ev_a, ev_b, NE, EvLess(), s); })))
    return e;
  // (ev_a is free: the unique keys go there; hull takes the survivors, candrod's last word their count)
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::reduce_by_key(t, b, (const Ev*)ev_b, (const Ev*)ev_b, NE, ev_a, hull, candrod + NE, Hull(),
                                       EvSame{multi}, s);
       })))
    return e;
  int64_t n_out = 0;
  HIP_TRY(hipMemcpyAsync(&n_out, candrod + NE, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // (the host vectors of the fold were read by now, too)
  const size_t NO = (size_t)n_out, NT = (size_t)n_t;
  uint32_t *isi, *islot;
  int64_t* res;
  if ((e = need(A.isi, &isi, NO + 1, "targets' ranges")) || (e = need(A.islot, &islot, NO + 1, "targets' ranges")) ||
      (e = need(A.res, &res, 7 * NO + 2 * (NT + 1), "targets' ranges")))
    return e;
  A.D = Result{res, res + NO, res + 2 * NO, res + 3 * NO, res + 4 * NO, res + 5 * NO, res + 6 * NO, res + 7 * NO,
               res + 7 * NO + NT + 1};
  JOB_TRY(launch(rt_isindel, grid(n_out), kThreads, s, hull, n_out, isi));
  if ((e = prim([&](void* t, size_t& b) {
         return rocprim::exclusive_scan(t, b, isi, islot, (uint32_t)0, NO + 1, rocprim::plus<uint32_t>(), s);
       })))
    return e;
  JOB_TRY(launch(rt_write, grid(n_out), kThreads, s, hull, islot, n_out, A.D));
  JOB_TRY(launch(rt_offsets, grid(n_t + 1), kThreads, s, hull, islot, n_out, n_t, A.D));
  HIP_TRY(A.clock.mark(RT_SETS_1, s));
  uint32_t n_indels = 0;
  HIP_TRY(hipMemcpyAsync(&n_indels, islot + n_out, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  upto_rods();
  A.clock.add(g_realign_ms[RT_CANDIDATES], RT_CANDIDATES_0, RT_CANDIDATES_1);
  A.clock.add(g_realign_ms[RT_SETS], RT_SETS_0, RT_SETS_1);
  A.sizes.n_candidates = n_cand;
  A.sizes.n_targets = n_t;
  A.sizes.n_indels = n_indels;
  A.sizes.n_snps = n_out - (int64_t)n_indels;
  return done();
}

bqsr_status rt_fetch(RtState& A, const bqsr_realign_targets_host* dst, hipStream_t s, const char* who) {
  if (!A.prepared) return fail(BQSR_ERR_INVALID_ARG, std::string(who) + " before its prepare call");
  const size_t nt = (size_t)A.sizes.n_targets, ni = (size_t)A.sizes.n_indels, ns = (size_t)A.sizes.n_snps;
  if (dst->target_start && nt) memcpy(dst->target_start, A.t_start.data(), nt * 8);
  if (dst->target_end && nt) memcpy(dst->target_end, A.t_end.data(), nt * 8);
  if (nt == 0) {  // no target: the two offset columns are their one 0
    if (dst->indel_offset) dst->indel_offset[0] = 0;
    if (dst->snp_offset) dst->snp_offset[0] = 0;
    return ok();
  }
  auto cp = [&](int64_t* d, const int64_t* src, size_t count) -> hipError_t {
    if (!d || !count) return hipSuccess;
    return hipMemcpyAsync(d, src, count * 8, hipMemcpyDeviceToHost, s);
  };
  hipError_t e = cp(dst->indel_offset, A.D.indel_offset, nt + 1);
  if (e == hipSuccess) e = cp(dst->snp_offset, A.D.snp_offset, nt + 1);
  if (e == hipSuccess) e = cp(dst->indel_start, A.D.indel_start, ni);
  if (e == hipSuccess) e = cp(dst->indel_end, A.D.indel_end, ni);
  if (e == hipSuccess) e = cp(dst->indel_read_start, A.D.indel_read_start, ni);
  if (e == hipSuccess) e = cp(dst->indel_read_end, A.D.indel_read_end, ni);
  if (e == hipSuccess) e = cp(dst->snp_site, A.D.snp_site, ns);
  if (e == hipSuccess) e = cp(dst->snp_read_start, A.D.snp_read_start, ns);
  if (e == hipSuccess) e = cp(dst->snp_read_end, A.D.snp_read_end, ns);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(BQSR_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
  return ok();
}

}  // namespace

extern "C" {

bqsr_status bqsr_sam_realign_targets_prepare(bqsr_context* ctx, bqsr_sam* s, void* stream,
                                             bqsr_realign_targets_sizes* out) {
  if (!ctx || !s || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_realign_targets_prepare: bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  return rt_prepare(ctx, *job_state<RtState>(s->realign_targets), pileup_view(s), S(stream), out);
}

bqsr_status bqsr_sam_realign_targets_fetch(bqsr_context* ctx, bqsr_sam* s, const bqsr_realign_targets_host* dst,
                                           void* stream) {
  if (!ctx || !s || !dst) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_realign_targets_fetch: bad arguments");
  if (!s->realign_targets)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_realign_targets_fetch before bqsr_sam_realign_targets_prepare");
  HIP_TRY(hipSetDevice(ctx->device));
  return rt_fetch(*job_state<RtState>(s->realign_targets), dst, S(stream), "bqsr_sam_realign_targets_fetch");
}

bqsr_status bqsr_arrow_realign_targets_prepare(bqsr_context* ctx, bqsr_arrow* a, void* stream,
                                               bqsr_realign_targets_sizes* out) {
  if (!ctx || !a || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_realign_targets_prepare: bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  // (mapq is no part of a target: the view's mapq columns are never read)
  return rt_prepare(ctx, *job_state<RtState>(a->realign_targets), pileup_view(a, *job_state<PileupState>(a->pileup)),
                    S(stream), out);
}

bqsr_status bqsr_arrow_realign_targets_fetch(bqsr_context* ctx, bqsr_arrow* a, const bqsr_realign_targets_host* dst,
                                             void* stream) {
  if (!ctx || !a || !dst) return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_realign_targets_fetch: bad arguments");
  if (!a->realign_targets)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_arrow_realign_targets_fetch before bqsr_arrow_realign_targets_prepare");
  HIP_TRY(hipSetDevice(ctx->device));
  return rt_fetch(*job_state<RtState>(a->realign_targets), dst, S(stream), "bqsr_arrow_realign_targets_fetch");
}

bqsr_status bqsr_realign_targets_kernel_times(double* ms7) {
  if (!ms7) return fail(BQSR_ERR_INVALID_ARG, "bqsr_realign_targets_kernel_times: null");
  for (int k = 0; k < RT_STAGES; ++k) ms7[k] = g_realign_ms[k];
  return BQSR_OK;
}

}  // extern "C"
