// `adam compare` and `adam findreads` on the device (include/adam_sam.h
// bqsr_compare_*): two inputs resident at once (each a bqsr_sam parse or a
// bqsr_arrow load, seen through one Side view), their reads bucketed by
// (recordGroupId, readName), the buckets joined by readName, and the five
// comparisons of metrics/AvailableComparisons.scala:44-177 aggregated into
// histograms (util/Histogram.scala).
//
// Passes (a lane per element unless said otherwise; every count is an
// integer sum, so no result depends on the schedule):
//   1. per side: mark_duplicates.hip's bucketing -- FNV-1a keys of (rg,
//      QNAME), radix sort with the read index (stable: a bucket's reads stay
//      in input order), run heads, every read's name bytes compared with its
//      run head's (a mismatch is a hash collision: status `collision`, the
//      caller decides) -- then a descriptor per bucket: the seven category
//      counts of models/ReadBucket.scala:97-110, the first read of each of
//      the five visited categories, allReads.head, the bucket's first read,
//      and a 64-bit FNV-1a of the name alone.
//   2. join: side 2's name hashes sorted with the bucket id; a lane per
//      bucket of side 1 finds its run of equal hashes by binary search and
//      accepts a candidate only when the name bytes are equal (a collision
//      costs a compare, nothing else); count, scan, emit the pair list.  The
//      uniques come from the same pass.
//   3. scalars: a lane per joined pair -- overmatched, positions (the -1
//      sentinels add into the sum), the mask of singly matched categories;
//      its popcounts scanned give the work list of matched read pairs, and a
//      lane per work item does dupemismatch, mapqs and min(len1, len2).
//      The two small histograms are counters fed by ballots, one atomic per
//      wave and counter; positions and mapqs are unbounded, so their values
//      go to arrays that rocprim sorts and run-length-encodes.
//   4. baseqs: the chars of the work items, scanned, are one index space cut
//      into chunks of kChunk chars; a workgroup takes chunks, each wavefront
//      kChunk / 8 consecutive chars of it, walking the read pairs that cover
//      them 64 chars a step -- both qual columns load contiguously and the
//      balance is by chars, not by pairs.  Points whose two low bytes are
//      below 128 go to a workgroup-private 128 x 128 table of u32 in LDS
//      (64 KB), the others straight to the 256 x 256 table of u64 in global
//      memory.  A workgroup counts the chars it took since its last flush
//      and flushes (64-bit global adds of the non-zero cells) before that
//      count could pass flush_chars < 2^32: no private counter can wrap.
//      A UTF-8 SAM / BAM side is decoded to char low bytes by a pass of its
//      own before the walk (a wavefront per read; its time counts as baseqs time),
//      so the walk is the same for both encodings; an Arrow side's quals are
//      the load's char low bytes already.
//   5. findreads: pair-level terms are evaluated in pass 3, dupemismatch /
//      mapqs terms per work item and baseqs terms inside pass 4, each setting
//      its bit of the pair's flag word; a predicate pass marks the pairs with
//      every bit set, one rocprim::select compacts their indices and a radix
//      sort orders them by (bucket 1's first read, bucket 2's first read).
//
// Included by bqsr_capi.cpp after pileup.hip.

namespace cmpk {

constexpr int kThreads = 256;
constexpr int kBqThreads = 512;            // pass 4: 8 wavefronts share one LDS table
constexpr int kBqWaves = kBqThreads / 64;
constexpr int kSub = 2048;                 // chars a wavefront takes of a chunk
constexpr int64_t kChunk = (int64_t)kSub * kBqWaves;
constexpr int kDense = 128;                // the LDS table's side
constexpr int kMaxTerms = 16;
constexpr int kVisited = 5;
enum { kOver = 0, kDupe = 1, kPos = 2, kMapq = 3, kBaseq = 4 };
enum { kEq = 0, kNe = 1, kLt = 2, kGt = 3 };

// ReadBucket's categories in allReads order; the five visited ones are 0, 1, 2, 4, 5
__device__ __forceinline__ int category(uint32_t raw_flag) {
  if (raw_flag == 0 || (raw_flag & 0x4)) return 6;  // FLAG 0: every boolean false (quirk Q2)
  const bool paired = raw_flag & 0x1, first = paired && (raw_flag & 0x40);
  const int k = first ? 1 : paired ? 2 : 0;
  return (raw_flag & 0x100) ? 3 + k : k;
}
__device__ __forceinline__ int visited_cat(int k) { return k < 3 ? k : k + 1; }

struct Desc {
  uint32_t cnt[7];
  uint32_t first[kVisited];  // the first read of visited category k (valid when its count > 0)
  uint32_t head;             // allReads.head
  uint32_t first_read;       // the bucket's first read in input order
};

struct Side {
  mdupd::DevSam S;
  const uint8_t* cat;       // [n] the read's ReadBucket category (cmp_cat_sam / cmp_arrow_chunk)
  const uint64_t* qual_span; // SAM text: the QUAL field of the line (null: the qual column, S.qual_off)
  const uint8_t* qbase;     // where the quals' char low bytes are: the text, the decoded buffer, the qual column
  const uint32_t* qlen;     // decoded side: chars per read
  const int32_t* mapq;      // Arrow side: mapq and whether it is set (null: parsed from the line)
  const uint8_t* mapq_ok;
  const uint32_t* idx;      // reads in bucket order
  const uint32_t* head_pos; // [nb]
  const Desc* desc;
  int64_t nb;
};

__device__ __forceinline__ uint64_t mask_bits(uint64_t h, int bits);
__device__ __forceinline__ int category_of(bool mapped, bool primary, bool paired, bool first) {
  if (!mapped) return 6;
  const int k = paired && first ? 1 : paired ? 2 : 0;
  return primary ? k : 3 + k;
}

extern "C" __global__ void __launch_bounds__(kThreads) cmp_cat_sam(const uint32_t* raw_flag, int64_t n, uint8_t* cat) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    cat[i] = (uint8_t)category(raw_flag[i]);
}

__device__ __forceinline__ bool bitmap_bit(const uint8_t* bm, int64_t i) { return (bm[i >> 3] >> (i & 7)) & 1u; }

// one Arrow chunk's firstOfPair and mapq columns (device copies of the host buffers) into the
// per-read columns of the side, rows [base, base + m): a null boolean reads as false
extern "C" __global__ void __launch_bounds__(kThreads) cmp_arrow_chunk(const uint32_t* flags, const uint8_t* first,
                                                                      const uint8_t* first_valid, const int32_t* mapq,
                                                                      const uint8_t* mapq_valid, int64_t m,
                                                                      int64_t base, uint8_t* cat, int32_t* out_mapq,
                                                                      uint8_t* out_ok) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t f = flags[base + i];
    const bool fp = first && (!first_valid || bitmap_bit(first_valid, i)) && bitmap_bit(first, i);
    cat[base + i] = (uint8_t)category_of(f & BQSR_F_MAPPED, f & BQSR_F_PRIMARY, f & BQSR_F_PAIRED, fp);
    const bool ok = mapq && (!mapq_valid || bitmap_bit(mapq_valid, i));
    out_mapq[base + i] = ok ? mapq[i] : 0;
    out_ok[base + i] = ok;
  }
}

// a null readName is a name of its own: its keys differ from those of ""
extern "C" __global__ void __launch_bounds__(kThreads) cmp_null_name_keys(const uint8_t* name_valid, const uint32_t* idx,
                                                                         uint64_t* key, int64_t n, int bits) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (!name_valid[idx[i]]) key[i] = mask_bits(key[i] ^ 0x9E3779B97F4A7C15ull, bits);
}

// after mdup_verify: a run that mixes a null readName with "" is a collision too
extern "C" __global__ void __launch_bounds__(kThreads) cmp_verify_null(const uint8_t* name_valid, const uint32_t* idx,
                                                                      const uint32_t* incl, const uint32_t* head_pos,
                                                                      int64_t n, int* bad) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (name_valid[idx[i]] != name_valid[idx[head_pos[incl[i] - 1]]]) atomicOr(bad, 1);
}

__device__ __forceinline__ uint64_t mask_bits(uint64_t h, int bits) { return bits >= 64 ? h : h & ((1ull << bits) - 1ull); }

extern "C" __global__ void __launch_bounds__(kThreads) cmp_mask_keys(uint64_t* key, int64_t n, int bits) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    key[i] = mask_bits(key[i], bits);
}

// strict UTF-8 -> the low bytes of the Java chars (a 4-byte sequence is a surrogate pair).  A
// wavefront per read, 64 bytes a step: a lane holding a lead byte checks and decodes its
// sequence; a lane holding a continuation byte checks that a lead within three bytes before
// it claims it; ballots of the leads give each char its place in the output.
extern "C" __global__ void __launch_bounds__(kThreads) cmp_decode_utf8(const uint8_t* text, const uint64_t* qual_span,
                                                                      const uint64_t* qual_off, int64_t n,
                                                                      uint8_t* out, uint32_t* qlen,
                                                                      unsigned long long* bad_read) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int64_t r = wave0; r < n; r += waves) {
    const uint8_t* p = text + qual_span[2 * r];
    const int64_t m = (int64_t)(qual_span[2 * r + 1] - qual_span[2 * r]);
    uint8_t* o = out + qual_off[r];  // (chars <= bytes: the read's slot of the parse's qual column layout)
    uint32_t k = 0;
    bool bad = false;
    for (int64_t i0 = 0; i0 < m; i0 += 64) {
      const int64_t i = i0 + lane;
      const bool live = i < m;
      const uint32_t b0 = live ? p[i] : 0u;
      const bool lead = live && (b0 & 0xC0u) != 0x80u;
      uint32_t cp = b0;
      bool good = true;
      if (lead) {
        int need = 0;
        uint32_t lo = 0x80, hi = 0xBF;
        if (b0 < 0x80) need = 0;
        else if (b0 >= 0xC2 && b0 <= 0xDF) need = 1, cp = b0 & 0x1F;
        else if (b0 >= 0xE0 && b0 <= 0xEF) {
          need = 2, cp = b0 & 0x0F;
          if (b0 == 0xE0) lo = 0xA0;
          if (b0 == 0xED) hi = 0x9F;
        } else if (b0 >= 0xF0 && b0 <= 0xF4) {
          need = 3, cp = b0 & 0x07;
          if (b0 == 0xF0) lo = 0x90;
          if (b0 == 0xF4) hi = 0x8F;
        } else good = false;
        if (good && i + need >= m) good = need == 0;  // a sequence cut off by the field's end
        if (good)
          for (int j = 1; j <= need; ++j) {
            const uint32_t c = p[i + j];
            if (c < (j == 1 ? lo : 0x80u) || c > (j == 1 ? hi : 0xBFu)) good = false;
            cp = (cp << 6) | (c & 0x3F);
          }
      } else if (live) {  // a continuation byte: the lead j bytes before it must take at least j more
        int j = 1;
        while (j <= 3 && i - j >= 0 && (p[i - j] & 0xC0u) == 0x80u) ++j;
        const uint32_t l = j <= 3 && i - j >= 0 ? p[i - j] : 0u;
        const int need = l >= 0xF0 ? 3 : l >= 0xE0 ? 2 : l >= 0xC0 ? 1 : 0;
        good = need >= j;
      }
      bad = bad || !good;
      // only checked sequences take a place: a good lead's followers are continuation bytes, which
      // take none, so the chars before a byte never outnumber the bytes before it (a bad lead --
      // 0xF5..0xFF, or 0xF1 before ASCII -- takes no place and fails the read)
      const bool one = lead && good, two = one && cp > 0xFFFF;
      const uint64_t m1 = __builtin_amdgcn_ballot_w64(one), m2 = __builtin_amdgcn_ballot_w64(two);
      const uint32_t at = k + (uint32_t)__popcll(m1 & below) + (uint32_t)__popcll(m2 & below);
      if (one && (int64_t)at + (two ? 1 : 0) < m) {  // (the bound holds by the count above; kept as a guard)
        if (two) {
          const uint32_t v = cp - 0x10000;
          o[at] = (uint8_t)((0xD800u + (v >> 10)) & 0xFF);
          o[at + 1] = (uint8_t)((0xDC00u + (v & 0x3FF)) & 0xFF);
        } else {
          o[at] = (uint8_t)(cp & 0xFF);
        }
      }
      k += (uint32_t)__popcll(m1) + (uint32_t)__popcll(m2);
    }
    const uint64_t any_bad = __builtin_amdgcn_ballot_w64(bad);
    if (lane == 0) {
      qlen[r] = k;
      if (any_bad) atomicMin(bad_read, (unsigned long long)r);
    }
  }
}

// pass 1: a lane per bucket
extern "C" __global__ void __launch_bounds__(kThreads) cmp_desc(mdupd::DevSam S, const uint8_t* cat,
                                                               const uint32_t* idx, const uint32_t* head_pos,
                                                               int64_t nb, int hash_bits, Desc* desc, uint64_t* nhash) {
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < nb; b += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = head_pos[b], i1 = b + 1 < nb ? (int64_t)head_pos[b + 1] : S.n;
    Desc d;
    uint32_t first7[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) d.cnt[c] = 0, first7[c] = 0;
    for (int64_t i = i0; i < i1; ++i) {
      const uint32_t r = idx[i];
      const int c = cat[r];
#pragma unroll
      for (int k = 0; k < 7; ++k)
        if (k == c) {
          if (d.cnt[k] == 0) first7[k] = r;
          ++d.cnt[k];
        }
    }
    d.head = idx[i0];
    bool found = false;
#pragma unroll
    for (int c = 0; c < 7; ++c)
      if (!found && d.cnt[c]) d.head = first7[c], found = true;
#pragma unroll
    for (int k = 0; k < kVisited; ++k) d.first[k] = first7[visited_cat(k)];
    d.first_read = idx[i0];  // the run is in input order
    desc[b] = d;
    const uint8_t* p;
    const int len = mdupd::name_len(S, (int64_t)idx[i0], &p);
    uint64_t h = 0xcbf29ce484222325ull;
    for (int i = 0; i < len; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    if (S.name_valid && !S.name_valid[idx[i0]]) h ^= 0x9E3779B97F4A7C15ull;  // a null readName
    nhash[b] = mask_bits(h, hash_bits);
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) cmp_iota(int64_t n, uint32_t* v) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    v[i] = (uint32_t)i;
}

__device__ __forceinline__ bool same_name(const mdupd::DevSam& A, int64_t ra, const mdupd::DevSam& B, int64_t rb) {
  const uint8_t *p, *q;
  const bool va = !A.name_valid || A.name_valid[ra], vb = !B.name_valid || B.name_valid[rb];
  if (va != vb) return false;  // null equals null only
  const int k = mdupd::name_len(A, ra, &p), m = mdupd::name_len(B, rb, &q);
  if (k != m) return false;
  for (int i = 0; i < k; ++i)
    if (p[i] != q[i]) return false;
  return true;
}

// first index of the sorted hashes not below h
__device__ __forceinline__ int64_t lower_bound(const uint64_t* v, int64_t n, uint64_t h) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (v[mid] < h) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// pass 2: kEmit = false counts the matches of each bucket of side 1 (and marks
// the matched buckets of side 2), kEmit = true writes the pairs at off[b]
template <bool kEmit>
__device__ __forceinline__ void join_walk(const Side& A, const Side& B, const uint64_t* nh1, const uint64_t* nh2s,
                                          const uint32_t* bid2s, int64_t b, unsigned long long* cnt,
                                          const unsigned long long* off, uint32_t* matched2, uint32_t* p1,
                                          uint32_t* p2) {
  const uint64_t h = nh1[b];
  const int64_t ra = A.idx[A.head_pos[b]];
  unsigned long long k = 0;
  for (int64_t j = lower_bound(nh2s, B.nb, h); j < B.nb && nh2s[j] == h; ++j) {
    const uint32_t b2 = bid2s[j];
    if (!same_name(A.S, ra, B.S, (int64_t)B.idx[B.head_pos[b2]])) continue;
    if (kEmit) {
      p1[off[b] + k] = (uint32_t)b;
      p2[off[b] + k] = b2;
    } else {
      matched2[b2] = 1u;
    }
    ++k;
  }
  if (!kEmit) cnt[b] = k;
}

extern "C" __global__ void __launch_bounds__(kThreads) cmp_join_count(Side A, Side B, const uint64_t* nh1,
                                                                     const uint64_t* nh2s, const uint32_t* bid2s,
                                                                     unsigned long long* cnt, uint32_t* matched2) {
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < A.nb; b += (int64_t)gridDim.x * blockDim.x)
    join_walk<false>(A, B, nh1, nh2s, bid2s, b, cnt, nullptr, matched2, nullptr, nullptr);
}

extern "C" __global__ void __launch_bounds__(kThreads) cmp_join_emit(Side A, Side B, const uint64_t* nh1,
                                                                    const uint64_t* nh2s, const uint32_t* bid2s,
                                                                    const unsigned long long* off, uint32_t* p1,
                                                                    uint32_t* p2) {
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < A.nb; b += (int64_t)gridDim.x * blockDim.x)
    join_walk<true>(A, B, nh1, nh2s, bid2s, b, nullptr, off, nullptr, p1, p2);
}

// unique buckets: side 1 those without a match, side 2 those never marked
extern "C" __global__ void __launch_bounds__(kThreads) cmp_uniques(const unsigned long long* cnt, int64_t nb1,
                                                                  const uint32_t* matched2, int64_t nb2,
                                                                  unsigned long long* out) {
  unsigned long long u1 = 0, u2 = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nb1; i += (int64_t)gridDim.x * blockDim.x)
    u1 += cnt[i] == 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nb2; i += (int64_t)gridDim.x * blockDim.x)
    u2 += matched2[i] == 0;
  for (int d = 32; d > 0; d >>= 1) {
    u1 += __shfl_xor(u1, d);
    u2 += __shfl_xor(u2, d);
  }
  if ((threadIdx.x & 63) == 0) {
    if (u1) atomicAdd(&out[0], u1);
    if (u2) atomicAdd(&out[1], u2);
  }
}

struct Term {
  int32_t comparison, op;
  int64_t a, b;
};
struct Terms {
  Term t[kMaxTerms];
  int32_t n;
};

__device__ __forceinline__ bool point_passes(const Term& t, int64_t x, int64_t y) {
  const bool eq = x == t.a && y == t.b;
  return t.op == kEq ? eq : !eq;
}

// the device counters: [0,2) overmatched false / true, [2,6) dupemismatch
// (d1, d2), [6,12) the first NULL_FIELD read of (comparison - kPos, side),
// [12] flushes, [13] unique1, [14] unique2, [15] bad UTF-8 read side 1, [16] side 2
enum { kCOver = 0, kCDupe = 2, kCNull = 6, kCFlush = 12, kCUnique = 13, kCBadUtf = 15, kCounters = 17 };

// one atomic per wave for a counter every lane may add one to
__device__ __forceinline__ void wave_add(unsigned long long* c, bool mine) {
  const uint64_t m = __builtin_amdgcn_ballot_w64(mine);
  if (m && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(m)) atomicAdd(c, (unsigned long long)__popcll(m));
}

// pass 3a: a lane per joined pair
extern "C" __global__ void __launch_bounds__(kThreads) cmp_pairs(Side A, Side B, const uint32_t* p1, const uint32_t* p2,
                                                                int64_t np, uint32_t want, Terms T, uint8_t* pmask,
                                                                unsigned long long* nwork, int64_t* posval,
                                                                uint32_t* pflag, unsigned long long* ctr) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); base < np; base += stride) {
    const int64_t p = base + lane;
    const bool live = p < np;
    bool over = true;
    uint32_t mask = 0, flag = 0;
    int64_t pos = 0;
    if (live) {
      const Desc d1 = A.desc[p1[p]], d2 = B.desc[p2[p]];
#pragma unroll
      for (int k = 0; k < kVisited; ++k) {
        const uint32_t c1 = d1.cnt[visited_cat(k)], c2 = d2.cnt[visited_cat(k)];
        over = over && c1 == c2 && c1 <= 1;
        const bool single = c1 == 1 && c2 == 1;
        if (single) mask |= 1u << k;
        if (want & (1u << kPos)) {
          if (single) {
            const uint32_t r1 = d1.first[k], r2 = d2.first[k];
            if (A.S.sq_id[r1] == B.S.sq_id[r2]) {  // null (-1) equals null
              const bool s1 = A.S.flags[r1] & BQSR_F_HAS_START, s2 = B.S.flags[r2] & BQSR_F_HAS_START;
              if (!s1) atomicMin(&ctr[kCNull + 0], (unsigned long long)r1);
              if (!s2) atomicMin(&ctr[kCNull + 1], (unsigned long long)r2);
              if (s1 && s2) {
                const int64_t a = A.S.start[r1], b = B.S.start[r2];
                pos += a > b ? a - b : b - a;
              }
            } else {
              pos -= 1;
            }
          } else if (c1 | c2) {
            pos -= 1;  // unequal sizes, or more than one read on both sides
          }
        }
      }
      for (int t = 0; t < T.n; ++t) {
        const Term& q = T.t[t];
        bool ok = false;
        if (q.comparison == kOver) ok = (over ? 1 : 0) == q.a;
        else if (q.comparison == kPos) ok = q.op == kEq ? pos == q.a : q.op == kLt ? pos < q.a : pos > q.a;
        if (ok) flag |= 1u << t;
      }
      pmask[p] = (uint8_t)mask;
      nwork[p] = (unsigned long long)__popc(mask);
      if (want & (1u << kPos)) posval[p] = pos;
      pflag[p] = flag;
    }
    if (want & (1u << kOver)) {
      wave_add(&ctr[kCOver + 0], live && !over);
      wave_add(&ctr[kCOver + 1], live && over);
    }
  }
}

struct Items {
  uint32_t *r1, *r2, *pair;
  unsigned long long *q1, *q2;   // where each read's chars begin in its side's qbase
  unsigned long long* len;       // min(len1, len2); scanned in place into the char offsets
  unsigned long long* mkey;      // (mapq1, mapq2)
};

// pass 3b: a lane per joined pair writes its work items
extern "C" __global__ void __launch_bounds__(kThreads) cmp_items(Side A, Side B, const uint32_t* p1, const uint32_t* p2,
                                                                int64_t np, const uint8_t* pmask,
                                                                const unsigned long long* woff, Items I) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < np; p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t mask = pmask[p];
    if (!mask) continue;
    const Desc& d1 = A.desc[p1[p]];
    const Desc& d2 = B.desc[p2[p]];
    unsigned long long w = woff[p];
    for (int k = 0; k < kVisited; ++k)
      if (mask & (1u << k)) {
        I.r1[w] = d1.first[k];
        I.r2[w] = d2.first[k];
        I.pair[w] = (uint32_t)p;
        ++w;
      }
  }
}

__device__ __forceinline__ bool read_mapq(const Side& X, uint32_t r, int64_t* mapq) {
  if (X.mapq_ok) {
    *mapq = X.mapq[r];
    return X.mapq_ok[r];
  }
  const uint8_t* t = X.S.text;
  const int64_t e = (int64_t)X.S.line_span[2 * (int64_t)r + 1];
  int64_t p = (int64_t)X.S.line_span[2 * (int64_t)r], a = 0, b = 0;
  for (int k = 0; k < 5; ++k) {  // MAPQ is field 5 of the line
    a = p;
    while (p < e && t[p] != '\t') ++p;
    b = p;
    if (p < e) ++p;
  }
  return adamk::mapq_field(t, a, b, X.S.sq_id[r], mapq);
}

__device__ __forceinline__ void read_quals(const Side& X, uint32_t r, unsigned long long* beg, unsigned long long* len) {
  if (X.qlen) {
    *beg = X.S.qual_off[r];
    *len = X.qlen[r];
  } else if (!X.qual_span) {
    *beg = X.S.qual_off[r];
    *len = X.S.qual_off[(int64_t)r + 1] - X.S.qual_off[r];
  } else {
    *beg = X.qual_span[2 * (int64_t)r];
    *len = X.qual_span[2 * (int64_t)r + 1] - X.qual_span[2 * (int64_t)r];
  }
}

// pass 3c: a lane per work item
extern "C" __global__ void __launch_bounds__(kThreads) cmp_item_values(Side A, Side B, int64_t nw, uint32_t want,
                                                                      Terms T, Items I, uint32_t* pflag,
                                                                      unsigned long long* ctr) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); base < nw; base += stride) {
    const int64_t w = base + lane;
    const bool live = w < nw;
    int d = -1;
    if (live) {
      const uint32_t r1 = I.r1[w], r2 = I.r2[w];
      uint32_t flag = 0;
      const int d1 = (A.S.flags[r1] & BQSR_F_DUPLICATE) ? 1 : 0, d2 = (B.S.flags[r2] & BQSR_F_DUPLICATE) ? 1 : 0;
      d = 2 * d1 + d2;
      int64_t m1 = 0, m2 = 0;
      if (want & (1u << kMapq)) {
        const bool h1 = read_mapq(A, r1, &m1), h2 = read_mapq(B, r2, &m2);
        if (!h1) atomicMin(&ctr[kCNull + 2], (unsigned long long)r1);
        if (!h2) atomicMin(&ctr[kCNull + 3], (unsigned long long)r2);
        I.mkey[w] = ((unsigned long long)(uint32_t)(int32_t)m1 << 32) | (unsigned long long)(uint32_t)(int32_t)m2;
      }
      unsigned long long len = 0;
      if (want & (1u << kBaseq)) {
        unsigned long long b1, l1, b2, l2;
        read_quals(A, r1, &b1, &l1);
        read_quals(B, r2, &b2, &l2);
        if (!(A.S.flags[r1] & BQSR_F_HAS_QUAL)) atomicMin(&ctr[kCNull + 4], (unsigned long long)r1);
        if (!(B.S.flags[r2] & BQSR_F_HAS_QUAL)) atomicMin(&ctr[kCNull + 5], (unsigned long long)r2);
        I.q1[w] = b1;
        I.q2[w] = b2;
        len = l1 < l2 ? l1 : l2;
      }
      I.len[w] = len;
      for (int t = 0; t < T.n; ++t) {
        const Term& q = T.t[t];
        if (q.comparison == kDupe && point_passes(q, d1, d2)) flag |= 1u << t;
        if (q.comparison == kMapq && point_passes(q, m1, m2)) flag |= 1u << t;
      }
      if (flag) atomicOr(&pflag[I.pair[w]], flag);
    }
    if (want & (1u << kDupe)) {
#pragma unroll
      for (int k = 0; k < 4; ++k) wave_add(&ctr[kCDupe + k], d == k);
    }
  }
}

struct BaseqArgs {
  const uint8_t *q1, *q2;             // the two sides' char low bytes
  const unsigned long long *b1, *b2;  // [nw] where a work item's chars begin
  const unsigned long long* coff;     // [nw + 1] the scanned char counts
  const uint32_t* pair;
  int64_t nw, chars, n_chunks, flush_chars;
  unsigned long long* table;          // 256 x 256
  uint32_t* pflag;
  unsigned long long* ctr;
  Terms T;
};

// pass 4
extern "C" __global__ void __launch_bounds__(kBqThreads) cmp_baseqs(BaseqArgs G) {
  __shared__ uint32_t tab[kDense * kDense];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < kDense * kDense; i += kBqThreads) tab[i] = 0;
  __syncthreads();
  auto flush = [&]() {
    __syncthreads();
    for (int i = threadIdx.x; i < kDense * kDense; i += kBqThreads) {
      const uint32_t v = tab[i];
      if (v) {
        atomicAdd(&G.table[(size_t)(i / kDense) * 256 + (size_t)(i % kDense)], (unsigned long long)v);
        tab[i] = 0;
      }
    }
    if (threadIdx.x == 0) atomicAdd(&G.ctr[kCFlush], 1ull);
    __syncthreads();
  };
  bool any_bq_term = false;
  for (int t = 0; t < G.T.n; ++t) any_bq_term |= G.T.t[t].comparison == kBaseq;
  int64_t taken = 0;  // chars this workgroup took since its last flush (the same value in every thread)
  for (int64_t c = blockIdx.x; c < G.n_chunks; c += gridDim.x) {
    if (taken + kChunk > G.flush_chars) {
      flush();
      taken = 0;
    }
    taken += kChunk;
    const int64_t a = c * kChunk + (int64_t)wave * kSub;
    const int64_t b = min(a + (int64_t)kSub, G.chars);
    if (a >= b) continue;  // (per wave; the barriers above are outside this)
    // the work item holding char a: the last w with coff[w] <= a
    int64_t lo = 0, hi = G.nw;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (G.coff[mid + 1] <= (unsigned long long)a) lo = mid + 1; else hi = mid;
    }
    int64_t w = lo, pos = a;
    while (pos < b && w < G.nw) {
      const int64_t s = (int64_t)G.coff[w], e = (int64_t)G.coff[w + 1];
      if (e <= pos) {
        ++w;
        continue;
      }
      const int64_t lim = min(e, b);
      const uint8_t* x = G.q1 + G.b1[w] + (pos - s);
      const uint8_t* y = G.q2 + G.b2[w] + (pos - s);
      const int64_t m = lim - pos;
      for (int64_t i0 = 0; i0 < m; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool live = i < m;
        uint32_t flag = 0;
        if (live) {
          const uint32_t u = (uint32_t)(uint8_t)(x[i] - 33), v = (uint32_t)(uint8_t)(y[i] - 33);
          if (u < (uint32_t)kDense && v < (uint32_t)kDense) atomicAdd(&tab[u * kDense + v], 1u);
          else atomicAdd(&G.table[(size_t)u * 256 + v], 1ull);
          if (any_bq_term) {
            const int64_t su = (int8_t)u, sv = (int8_t)v;
            for (int t = 0; t < G.T.n; ++t)
              if (G.T.t[t].comparison == kBaseq && point_passes(G.T.t[t], su, sv)) flag |= 1u << t;
          }
        }
        if (any_bq_term) {
          for (int d = 32; d > 0; d >>= 1) flag |= __shfl_xor(flag, d);
          if (flag && lane == 0) atomicOr(&G.pflag[G.pair[w]], flag);
        }
      }
      pos = lim;
      if (pos == e) ++w;
    }
  }
  flush();
}

// pass 5: the pairs with every term's bit set
extern "C" __global__ void __launch_bounds__(kThreads) cmp_predicate(const uint32_t* pflag, int64_t np,
                                                                    uint32_t all, uint8_t* pass) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < np; p += (int64_t)gridDim.x * blockDim.x)
    pass[p] = (pflag[p] & all) == all;
}

// the selected pairs' sort keys (first reads of the two buckets) and rows (their allReads.head reads)
extern "C" __global__ void __launch_bounds__(kThreads) cmp_row_keys(Side A, Side B, const uint32_t* p1,
                                                                   const uint32_t* p2, const uint32_t* sel, int64_t n,
                                                                   unsigned long long* key, unsigned long long* val) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const Desc& d1 = A.desc[p1[sel[i]]];
    const Desc& d2 = B.desc[p2[sel[i]]];
    key[i] = ((unsigned long long)d1.first_read << 32) | d2.first_read;
    val[i] = ((unsigned long long)d1.head << 32) | d2.head;
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) cmp_split_rows(const unsigned long long* val, int64_t n,
                                                                     uint32_t* h1, uint32_t* h2) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    h1[i] = (uint32_t)(val[i] >> 32);
    h2[i] = (uint32_t)val[i];
  }
}

}  // namespace cmpk

struct bqsr_compare {
  bqsr_context* ctx = nullptr;
  bqsr_compare_options opt{};
  // the last run's results, on the device
  std::vector<void*> keep;
  void* pos_val = nullptr;
  void* pos_cnt = nullptr;
  void* mapq_val = nullptr;
  void* mapq_cnt = nullptr;
  unsigned long long* table = nullptr;
  uint32_t *row1 = nullptr, *row2 = nullptr;
  int64_t n_pos = 0, n_mapq = 0, n_rows = 0;
  bool ran = false;
  // the last run's join, scalar and baseqs (+ UTF-8 decode) kernels (measurement only), and the clock's marks:
  // a begin and an end per stage, then per side's decode pass
  enum { JOIN, SCALAR, BASEQS, STAGES };
  enum { JOIN_0, JOIN_1, SCALAR_0, SCALAR_1, BASEQS_0, BASEQS_1, DECODE1_0, DECODE1_1, DECODE2_0, DECODE2_1, MARKS };
  StageClock<MARKS> clock;
  double ms[STAGES] = {0.0, 0.0, 0.0};
  bool decoded[2] = {false, false};
  void release() {
    for (void* p : keep) (void)hipFree(p);
    keep.clear();
    pos_val = pos_cnt = mapq_val = mapq_cnt = nullptr;
    table = nullptr;
    row1 = row2 = nullptr;
    n_pos = n_mapq = n_rows = 0;
    ran = false;
  }
  ~bqsr_compare() {
    release();
  }
};

namespace {


// host-only checks (no device call): the options and the filter terms
bqsr_status compare_check_options(const bqsr_compare_options* o) {
  if (!o) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: null options");
  if (o->hash_bits < 1 || o->hash_bits > 64) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: hash_bits outside [1, 64]");
  if ((o->utf8_1 | o->utf8_2) & ~1) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: utf8 flags are 0 or 1");
  if (o->comparisons >= (1u << 5)) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: unknown comparison bits");
  if (o->flush_chars < 0 || o->flush_chars > (int64_t)BQSR_COMPARE_MAX_FLUSH_CHARS)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: flush_chars outside [0, 2^31]");
  if (o->baseq_groups < 0 || o->reserved != 0)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: baseq_groups is negative, or reserved is not 0");
  if (o->flush_chars && o->flush_chars < cmpk::kChunk)
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: flush_chars below one chunk (16384 chars)");
  return BQSR_OK;
}

}  // namespace

extern "C" {

bqsr_status bqsr_compare_check_terms(const bqsr_compare_term* terms, int32_t n_terms) {
  using namespace cmpk;
  if (n_terms < 0 || (n_terms && !terms)) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: bad terms");
  if (n_terms > kMaxTerms) return fail(BQSR_ERR_UNSUPPORTED, "bqsr_compare: more than 16 filter terms");
  for (int32_t i = 0; i < n_terms; ++i) {
    const bqsr_compare_term& t = terms[i];
    if (t.comparison < kOver || t.comparison > kBaseq)
      return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: a term names no comparison");
    const bool is_bool = t.comparison == kOver, is_long = t.comparison == kPos;
    const bool legal = is_bool ? t.op == kEq : is_long ? (t.op == kEq || t.op == kLt || t.op == kGt)
                                                       : (t.op == kEq || t.op == kNe);
    if (!legal) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: the operator is not legal for the term's comparison");
    if (is_bool && (t.a < 0 || t.a > 1)) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: a boolean term takes 0 or 1");
    if (!is_bool && !is_long && (t.a < INT32_MIN || t.a > INT32_MAX || t.b < INT32_MIN || t.b > INT32_MAX))
      return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: a point term's values are 32-bit");
  }
  return ok();
}

bqsr_status bqsr_compare_create(bqsr_context* ctx, const bqsr_compare_options* options, bqsr_compare** out) {
  if (!out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare_create: null");
  *out = nullptr;
  bqsr_compare_options o{};
  o.hash_bits = 64;
  o.comparisons = 1u << cmpk::kBaseq;
  if (options) o = *options;
  if (o.hash_bits == 0) o.hash_bits = 64;
  const bqsr_status e = compare_check_options(&o);
  if (e != BQSR_OK) return e;
  if (!ctx) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare_create: null context");
  HIP_TRY(hipSetDevice(ctx->device));
  auto* c = new bqsr_compare();
  c->ctx = ctx;
  c->opt = o;
  if (c->clock.create() != hipSuccess) {
    delete c;
    return fail(BQSR_ERR_DEVICE, "bqsr_compare_create: hipEventCreate failed");
  }
  *out = c;
  return ok();
}

void bqsr_compare_destroy(bqsr_compare* c) { delete c; }

}  // extern "C"

namespace {

using cmp_ull = unsigned long long;

// one input's bucketing and descriptors (pass 1); every buffer lives in T
struct CompareSide {
  cmpk::Side D{};
  uint64_t* nhash = nullptr;
  int64_t nb = 0;
  bool collision = false;
};

// the Arrow side's firstOfPair and mapq chunks -> per-read columns (cat, mapq, mapq_ok)
bqsr_status compare_arrow_columns(bqsr_compare* c, const bqsr_compare_side* in, SortTmp& T, hipStream_t st,
                                  uint8_t* cat, int32_t* mapq, uint8_t* ok) {
  using namespace cmpk;
  const bqsr_arrow* a = in->arrow;
  if (in->n_chunks < 0 || (in->n_chunks && !in->chunk_reads))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: bad Arrow chunk list");
  int64_t tot = 0;
  for (int32_t k = 0; k < in->n_chunks; ++k) {
    if (in->chunk_reads[k] < 0) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: negative chunk length");
    tot += in->chunk_reads[k];
  }
  if (tot != a->n) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare: the firstOfPair / mapq chunks do not cover the reads");
  int64_t base = 0;
  bqsr_status e;
  for (int32_t k = 0; k < in->n_chunks; ++k) {
    const int64_t m = in->chunk_reads[k];
    if (m == 0) continue;
    const size_t vb = (size_t)(m + 7) / 8;
    const uint8_t* hf = in->first_of_pair ? in->first_of_pair[k] : nullptr;
    const uint8_t* hfv = hf && in->first_of_pair_validity ? in->first_of_pair_validity[k] : nullptr;
    const int32_t* hm = in->mapq ? in->mapq[k] : nullptr;
    const uint8_t* hmv = hm && in->mapq_validity ? in->mapq_validity[k] : nullptr;
    uint8_t *df = nullptr, *dfv = nullptr, *dmv = nullptr;
    int32_t* dm = nullptr;
    auto up = [&](auto** d, const void* h, size_t count) -> bqsr_status {
      if (!h) return BQSR_OK;
      bqsr_status x = sam_alloc(T.v, d, count);
      if (x != BQSR_OK) return x;
      HIP_TRY(hipMemcpyAsync(*d, h, count * sizeof(**d), hipMemcpyHostToDevice, st));
      return BQSR_OK;
    };
    if ((e = up(&df, hf, vb)) || (e = up(&dfv, hfv, vb)) || (e = up(&dm, hm, (size_t)m)) || (e = up(&dmv, hmv, vb)))
      return e;
    JOB_TRY(launch(cmp_arrow_chunk, sam_grid(m, kThreads, c->ctx->n_cu * 16), kThreads, st, a->flags, df, dfv, dm, dmv,
                   m, base, cat, mapq, ok));
    base += m;
  }
  HIP_TRY(hipStreamSynchronize(st));  // (the host buffers are the caller's: read before the call returns)
  return BQSR_OK;
}

bqsr_status compare_side(bqsr_compare* c, const bqsr_compare_side* in, bool utf8, int side, uint32_t want, SortTmp& T,
                         hipStream_t st, cmp_ull* ctr, CompareSide* out) {
  using namespace cmpk;
  const bqsr_sam* s = in->sam;
  const bqsr_arrow* a = in->arrow;
  const int64_t n = s ? s->n_reads : a->n;
  if (n > (int64_t)BQSR_COMPARE_MAX_READS)
    return fail(BQSR_ERR_UNSUPPORTED, "bqsr_compare: more than 2^32 - 1 reads in one input");
  mdupd::DevSam S{};
  Side& D = out->D;
  if (s) {
    S = mdupd::DevSam{s->d_text, s->line_span, s->flags, s->rg_id, s->sq_id, s->start, s->qual_off, s->qual,
                      s->cig_off, s->cig, nullptr, s->n_rg, n};
    D.qual_span = s->qual_span;
    D.qbase = s->d_text;
  } else {  // the columns bqsr_arrow_load built: names in their own buffer, quals already char low bytes
    S.text = a->raw[arwk::kName];
    S.flags = a->flags;
    S.rg_id = a->rg;
    S.sq_id = a->sq;
    S.start = a->start;
    S.qual_off = a->qual_off;
    S.qual = a->qual;
    S.cig_off = a->cig_off;
    S.cig = a->cig;
    S.n = n;
    S.name_beg = a->beg[arwk::kName];
    S.name_valid = a->name_valid;
    D.qual_span = nullptr;
    D.qbase = a->qual;
  }
  D.S = S;
  if (n == 0) return BQSR_OK;
  const unsigned g = sam_grid(n, kThreads, c->ctx->n_cu * 16);
  bqsr_status e;
  uint8_t* cat = nullptr;
  if ((e = sam_alloc(T.v, &cat, (size_t)n))) return e;
  if (s) {
    JOB_TRY(launch(cmp_cat_sam, g, kThreads, st, s->raw_flag, n, cat));
  } else {
    int32_t* mq = nullptr;
    uint8_t* ok = nullptr;
    if ((e = sam_alloc(T.v, &mq, (size_t)n)) || (e = sam_alloc(T.v, &ok, (size_t)n))) return e;
    if ((e = compare_arrow_columns(c, in, T, st, cat, mq, ok))) return e;
    D.mapq = mq;
    D.mapq_ok = ok;
  }
  D.cat = cat;
  if (s && utf8 && (want & (1u << kBaseq))) {
    uint8_t* dq = nullptr;
    uint32_t* qlen = nullptr;
    if ((e = sam_alloc(T.v, &dq, (size_t)s->qual_bytes)) || (e = sam_alloc(T.v, &qlen, (size_t)n))) return e;
    HIP_TRY(c->clock.mark(side ? bqsr_compare::DECODE2_0 : bqsr_compare::DECODE1_0, st));
    JOB_TRY(launch(cmp_decode_utf8, sam_grid(n, kThreads / 64, c->ctx->n_cu * 16), kThreads, st, s->d_text,
                   s->qual_span, s->qual_off, n, dq, qlen, ctr + kCBadUtf + side));
    HIP_TRY(c->clock.mark(side ? bqsr_compare::DECODE2_1 : bqsr_compare::DECODE1_1, st));
    c->decoded[side] = true;
    D.qbase = dq;
    D.qlen = qlen;
  }
  uint64_t *key = nullptr, *key2 = nullptr;
  uint32_t *idx = nullptr, *idx2 = nullptr, *head = nullptr, *incl = nullptr, *hpos = nullptr;
  int* bad = nullptr;
  const size_t N = (size_t)n;
  if ((e = sam_alloc(T.v, &key, N)) || (e = sam_alloc(T.v, &key2, N)) || (e = sam_alloc(T.v, &idx, N)) ||
      (e = sam_alloc(T.v, &idx2, N)) || (e = sam_alloc(T.v, &head, N)) || (e = sam_alloc(T.v, &incl, N)) ||
      (e = sam_alloc(T.v, &hpos, N)) || (e = sam_alloc(T.v, &bad, 1)))
    return e;
  HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), st));
  // mark_duplicates.hip's passes: keys, sort, heads, verify
  JOB_TRY(launch(mdupd::mdup_keys, g, mdupd::kThreads, st, S, key, idx));
  if (c->opt.hash_bits < 64) JOB_TRY(launch(cmp_mask_keys, g, kThreads, st, key, n, c->opt.hash_bits));
  if (S.name_valid)
    JOB_TRY(launch(cmp_null_name_keys, g, kThreads, st, S.name_valid, idx, key, n, c->opt.hash_bits));
  if ((e = with_temp(T.v, [&](void* t, size_t& b) {
         return rocprim::radix_sort_pairs(t, b, key, key2, idx, idx2, N, 0, 64, st);
       })))
    return e;
  JOB_TRY(launch(mdupd::mdup_heads, g, mdupd::kThreads, st, key2, n, head));
  if ((e = with_temp(T.v, [&](void* t, size_t& b) {
         return rocprim::inclusive_scan(t, b, head, incl, N, rocprim::plus<uint32_t>(), st);
       })))
    return e;
  JOB_TRY(launch(mdupd::mdup_head_pos, g, mdupd::kThreads, st, head, incl, n, hpos));
  JOB_TRY(launch(mdupd::mdup_verify, g, mdupd::kThreads, st, S, idx2, incl, hpos, bad));
  if (S.name_valid)
    JOB_TRY(launch(cmp_verify_null, g, kThreads, st, S.name_valid, idx2, incl, hpos, n, bad));
  uint32_t nb32 = 0;
  int hbad = 0;
  HIP_TRY(hipMemcpyAsync(&nb32, incl + (n - 1), 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  out->collision = hbad != 0;
  out->nb = nb32;
  if (out->collision) return BQSR_OK;
  Desc* desc = nullptr;
  if ((e = sam_alloc(T.v, &desc, (size_t)out->nb)) || (e = sam_alloc(T.v, &out->nhash, (size_t)out->nb))) return e;
  JOB_TRY(launch(cmp_desc, sam_grid(out->nb, kThreads, c->ctx->n_cu * 16), kThreads, st, S, cat, idx2, hpos, out->nb,
                 c->opt.hash_bits, desc, out->nhash));
  D.idx = idx2;
  D.head_pos = hpos;
  D.desc = desc;
  D.nb = out->nb;
  return BQSR_OK;
}

// sorted values -> (value, count) runs kept on the handle
template <class K>
bqsr_status compare_rle(bqsr_compare* c, SortTmp& T, hipStream_t st, K* vals, int64_t n, void** out_val,
                        void** out_cnt, int64_t* n_runs) {
  *n_runs = 0;
  if (n == 0) return BQSR_OK;
  K *sorted = nullptr, *uniq = nullptr;
  cmp_ull *cnt = nullptr, *runs = nullptr;
  bqsr_status e;
  if ((e = sam_alloc(T.v, &sorted, (size_t)n)) || (e = sam_alloc(c->keep, &uniq, (size_t)n)) ||
      (e = sam_alloc(c->keep, &cnt, (size_t)n)) || (e = sam_alloc(T.v, &runs, 1)))
    return e;
  if ((e = with_temp(T.v, [&](void* t, size_t& b) {
         return rocprim::radix_sort_keys(t, b, vals, sorted, (size_t)n, 0, 64, st);
       })))
    return e;
  if ((e = with_temp(T.v, [&](void* t, size_t& b) {
         return rocprim::run_length_encode(t, b, sorted, (unsigned int)n, uniq, cnt, runs, st);
       })))
    return e;
  cmp_ull h = 0;
  HIP_TRY(hipMemcpyAsync(&h, runs, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *out_val = uniq;
  *out_cnt = cnt;
  *n_runs = (int64_t)h;
  return BQSR_OK;
}

}  // namespace

extern "C" {

bqsr_status bqsr_compare_sam(bqsr_compare* c, const bqsr_sam* s1, const bqsr_sam* s2, const bqsr_compare_term* terms,
                             int32_t n_terms, void* stream, bqsr_compare_result* out) {
  if (!c || !s1 || !s2 || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare_sam: bad arguments");
  bqsr_compare_side a{}, b{};
  a.sam = s1;
  b.sam = s2;
  return bqsr_compare_sides(c, &a, &b, terms, n_terms, stream, out);
}

bqsr_status bqsr_compare_sides(bqsr_compare* c, const bqsr_compare_side* in1, const bqsr_compare_side* in2,
                               const bqsr_compare_term* terms, int32_t n_terms, void* stream,
                               bqsr_compare_result* out) {
  using namespace cmpk;
  if (!c || !in1 || !in2 || !out) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare_sides: bad arguments");
  for (const bqsr_compare_side* in : {in1, in2}) {
    if (!in->sam == !in->arrow) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare_sides: a side is one parse or one Arrow load");
    if ((in->sam ? in->sam->ctx : in->arrow->ctx) != c->ctx)
      return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare_sides: input of another context");
  }
  bqsr_status e = bqsr_compare_check_terms(terms, n_terms);
  if (e != BQSR_OK) return e;
  memset(out, 0, sizeof *out);
  out->null_comparison = -1;
  HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = S(stream);
  c->release();
  for (double& v : c->ms) v = 0.0;
  c->decoded[0] = c->decoded[1] = false;
  uint32_t want = c->opt.comparisons;
  Terms TT{};
  TT.n = n_terms;
  for (int32_t i = 0; i < n_terms; ++i) {
    TT.t[i] = Term{terms[i].comparison, terms[i].op, terms[i].a, terms[i].b};
    want |= 1u << terms[i].comparison;
  }
  SortTmp T;
  cmp_ull* ctr = nullptr;
  if ((e = sam_alloc(T.v, &ctr, kCounters))) return e;
  {
    cmp_ull h[kCounters];
    for (int i = 0; i < kCounters; ++i) h[i] = (i >= kCNull && i < kCNull + 6) || i >= kCBadUtf ? ~0ull : 0ull;
    HIP_TRY(hipMemcpyAsync(ctr, h, sizeof h, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (h leaves scope)
  }
  CompareSide A, B;
  e = compare_side(c, in1, c->opt.utf8_1 != 0, 0, want, T, st, ctr, &A);
  if (e == BQSR_OK) e = compare_side(c, in2, c->opt.utf8_2 != 0, 1, want, T, st, ctr, &B);
  if (e != BQSR_OK) return e;
  if (A.collision || B.collision) {
    out->collision = 1;
    return ok();
  }
  const int64_t nb1 = A.nb, nb2 = B.nb;
  out->total1 = nb1;
  out->total2 = nb2;
  const int cap = c->ctx->n_cu * 16;
  // ---- pass 2: the join
  int64_t np = 0;
  uint32_t *p1 = nullptr, *p2 = nullptr;
  cmp_ull *cnt = nullptr, *off = nullptr;
  uint32_t* matched2 = nullptr;
  HIP_TRY(c->clock.mark(bqsr_compare::JOIN_0, st));
  if ((e = sam_alloc(T.v, &cnt, (size_t)nb1)) || (e = sam_alloc(T.v, &off, (size_t)nb1)) ||
      (e = sam_alloc(T.v, &matched2, (size_t)nb2)))
    return e;
  HIP_TRY(hipMemsetAsync(matched2, 0, (size_t)std::max<int64_t>(nb2, 1) * 4, st));
  HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)std::max<int64_t>(nb1, 1) * 8, st));
  uint64_t* nh2s = nullptr;
  uint32_t *bid2 = nullptr, *bid2s = nullptr;
  if (nb1 && nb2) {
    if ((e = sam_alloc(T.v, &nh2s, (size_t)nb2)) || (e = sam_alloc(T.v, &bid2, (size_t)nb2)) ||
        (e = sam_alloc(T.v, &bid2s, (size_t)nb2)))
      return e;
    JOB_TRY(launch(cmp_iota, sam_grid(nb2, kThreads, cap), kThreads, st, nb2, bid2));
    if ((e = with_temp(T.v, [&](void* t, size_t& b) {
           return rocprim::radix_sort_pairs(t, b, B.nhash, nh2s, bid2, bid2s, (size_t)nb2, 0, 64, st);
         })))
      return e;
    JOB_TRY(launch(cmp_join_count, sam_grid(nb1, kThreads, cap), kThreads, st, A.D, B.D, A.nhash, nh2s, bid2s, cnt,
                   matched2));
    if ((e = with_temp(T.v, [&](void* t, size_t& b) {
           return rocprim::exclusive_scan(t, b, cnt, off, (cmp_ull)0, (size_t)nb1, rocprim::plus<cmp_ull>(), st);
         })))
      return e;
    cmp_ull last[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&last[0], cnt + (nb1 - 1), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last[1], off + (nb1 - 1), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (last[0] + last[1] > (cmp_ull)BQSR_COMPARE_MAX_READS)
      return fail(BQSR_ERR_UNSUPPORTED, "bqsr_compare: more than 2^32 - 1 joined pairs");
    np = (int64_t)(last[0] + last[1]);
    if (np) {
      if ((e = sam_alloc(T.v, &p1, (size_t)np)) || (e = sam_alloc(T.v, &p2, (size_t)np))) return e;
      JOB_TRY(launch(cmp_join_emit, sam_grid(nb1, kThreads, cap), kThreads, st, A.D, B.D, A.nhash, nh2s, bid2s, off, p1,
                     p2));
    }
  }
  if (nb1 + nb2) {
    JOB_TRY(launch(cmp_uniques, sam_grid(std::max(nb1, nb2), kThreads, cap), kThreads, st, cnt, nb1, matched2, nb2,
                   ctr + kCUnique));
  }
  HIP_TRY(c->clock.mark(bqsr_compare::JOIN_1, st));
  out->n_pairs = np;
  // ---- pass 3: scalars and the work list
  uint8_t* pmask = nullptr;
  cmp_ull *nwork = nullptr, *woff = nullptr;
  int64_t* posval = nullptr;
  uint32_t* pflag = nullptr;
  Items I{};
  int64_t nw = 0, chars = 0;
  cmp_ull* coff = nullptr;
  HIP_TRY(c->clock.mark(bqsr_compare::SCALAR_0, st));
  if (np) {
    if ((e = sam_alloc(T.v, &pmask, (size_t)np)) || (e = sam_alloc(T.v, &nwork, (size_t)np)) ||
        (e = sam_alloc(T.v, &woff, (size_t)np)) || (e = sam_alloc(T.v, &posval, (size_t)np)) ||
        (e = sam_alloc(T.v, &pflag, (size_t)np)))
      return e;
    const unsigned gp = sam_grid(np, kThreads, cap);
    JOB_TRY(launch(cmp_pairs, gp, kThreads, st, A.D, B.D, p1, p2, np, want, TT, pmask, nwork, posval, pflag, ctr));
    if ((e = with_temp(T.v, [&](void* t, size_t& b) {
           return rocprim::exclusive_scan(t, b, nwork, woff, (cmp_ull)0, (size_t)np, rocprim::plus<cmp_ull>(), st);
         })))
      return e;
    cmp_ull last[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&last[0], nwork + (np - 1), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last[1], woff + (np - 1), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (last[0] + last[1] > (cmp_ull)BQSR_COMPARE_MAX_READS)
      return fail(BQSR_ERR_UNSUPPORTED, "bqsr_compare: more than 2^32 - 1 matched read pairs");
    nw = (int64_t)(last[0] + last[1]);
  }
  if (nw) {
    const size_t W = (size_t)nw;
    if ((e = sam_alloc(T.v, &I.r1, W)) || (e = sam_alloc(T.v, &I.r2, W)) || (e = sam_alloc(T.v, &I.pair, W)) ||
        (e = sam_alloc(T.v, &I.q1, W)) || (e = sam_alloc(T.v, &I.q2, W)) || (e = sam_alloc(T.v, &I.len, W)) ||
        (e = sam_alloc(T.v, &I.mkey, W)) || (e = sam_alloc(T.v, &coff, W + 1)))
      return e;
    JOB_TRY(launch(cmp_items, sam_grid(np, kThreads, cap), kThreads, st, A.D, B.D, p1, p2, np, pmask, woff, I));
    JOB_TRY(launch(cmp_item_values, sam_grid(nw, kThreads, cap), kThreads, st, A.D, B.D, nw, want, TT, I, pflag, ctr));
  }
  HIP_TRY(c->clock.mark(bqsr_compare::SCALAR_1, st));
  // the unbounded histograms: sort and run-length-encode
  if ((want & (1u << kPos)) && np)
    if ((e = compare_rle<int64_t>(c, T, st, posval, np, &c->pos_val, &c->pos_cnt, &c->n_pos))) return e;
  if ((want & (1u << kMapq)) && nw)
    if ((e = compare_rle<cmp_ull>(c, T, st, I.mkey, nw, &c->mapq_val, &c->mapq_cnt, &c->n_mapq))) return e;
  // ---- pass 4: baseqs
  if ((e = sam_alloc(c->keep, &c->table, (size_t)256 * 256))) return e;
  HIP_TRY(hipMemsetAsync(c->table, 0, (size_t)256 * 256 * 8, st));
  if ((want & (1u << kBaseq)) && nw) {
    // coff[0] = 0, coff[w + 1] = the inclusive scan of the lengths
    HIP_TRY(hipMemsetAsync(coff, 0, 8, st));
    if ((e = with_temp(T.v, [&](void* t, size_t& b) {
           return rocprim::inclusive_scan(t, b, I.len, coff + 1, (size_t)nw, rocprim::plus<cmp_ull>(), st);
         })))
      return e;
    cmp_ull total = 0;
    HIP_TRY(hipMemcpyAsync(&total, coff + nw, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    chars = (int64_t)total;
  }
  HIP_TRY(c->clock.mark(bqsr_compare::BASEQS_0, st));
  if (chars) {
    BaseqArgs G{};
    G.q1 = A.D.qbase;
    G.q2 = B.D.qbase;
    G.b1 = I.q1;
    G.b2 = I.q2;
    G.coff = coff;
    G.pair = I.pair;
    G.nw = nw;
    G.chars = chars;
    G.n_chunks = (chars + cmpk::kChunk - 1) / cmpk::kChunk;
    G.flush_chars = c->opt.flush_chars ? c->opt.flush_chars : (int64_t)BQSR_COMPARE_MAX_FLUSH_CHARS;
    G.table = c->table;
    G.pflag = pflag;
    G.ctr = ctr;
    G.T = TT;
    const int64_t groups = c->opt.baseq_groups ? c->opt.baseq_groups : (int64_t)c->ctx->n_cu * 2;
    const unsigned gb = (unsigned)std::max<int64_t>(1, std::min<int64_t>(G.n_chunks, groups));
    JOB_TRY(launch(cmp_baseqs, gb, kBqThreads, st, G));
  }
  HIP_TRY(c->clock.mark(bqsr_compare::BASEQS_1, st));
  out->baseq_chars = chars;
  // ---- pass 5: findreads
  if (n_terms && np) {
    uint8_t* pass = nullptr;
    cmp_ull *skey = nullptr, *sval = nullptr, *okey = nullptr, *oval = nullptr;
    cmp_ull* nsel = nullptr;
    uint32_t* sel = nullptr;
    const size_t P = (size_t)np;
    if ((e = sam_alloc(T.v, &pass, P)) || (e = sam_alloc(T.v, &sel, P)) || (e = sam_alloc(T.v, &nsel, 1))) return e;
    const uint32_t all = n_terms >= 32 ? ~0u : (1u << n_terms) - 1u;
    JOB_TRY(launch(cmp_predicate, sam_grid(np, kThreads, cap), kThreads, st, pflag, np, all, pass));
    if ((e = with_temp(T.v, [&](void* t, size_t& b) {  // one select: the passing pairs' indices
           return rocprim::select(t, b, rocprim::counting_iterator<uint32_t>(0), pass, sel, nsel, P, st);
         })))
      return e;
    cmp_ull hs = 0;
    HIP_TRY(hipMemcpyAsync(&hs, nsel, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hs) {
      if ((e = sam_alloc(T.v, &skey, (size_t)hs)) || (e = sam_alloc(T.v, &sval, (size_t)hs)) ||
          (e = sam_alloc(T.v, &okey, (size_t)hs)) || (e = sam_alloc(T.v, &oval, (size_t)hs)))
        return e;
      JOB_TRY(launch(cmp_row_keys, sam_grid((int64_t)hs, kThreads, cap), kThreads, st, A.D, B.D, p1, p2, sel,
                     (int64_t)hs, skey, sval));
      if ((e = with_temp(T.v, [&](void* t, size_t& b) {
             return rocprim::radix_sort_pairs(t, b, skey, okey, sval, oval, (size_t)hs, 0, 64, st);
           })))
        return e;
      if ((e = sam_alloc(c->keep, &c->row1, (size_t)hs)) || (e = sam_alloc(c->keep, &c->row2, (size_t)hs))) return e;
      JOB_TRY(launch(cmp_split_rows, sam_grid((int64_t)hs, kThreads, cap), kThreads, st, oval, (int64_t)hs, c->row1,
                     c->row2));
    }
    c->n_rows = (int64_t)hs;
  }
  cmp_ull h[kCounters];
  HIP_TRY(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  c->clock.add(c->ms[bqsr_compare::JOIN], bqsr_compare::JOIN_0, bqsr_compare::JOIN_1);
  c->clock.add(c->ms[bqsr_compare::SCALAR], bqsr_compare::SCALAR_0, bqsr_compare::SCALAR_1);
  c->clock.add(c->ms[bqsr_compare::BASEQS], bqsr_compare::BASEQS_0, bqsr_compare::BASEQS_1);
  // a UTF-8 side's decode pass belongs to the baseqs time
  if (c->decoded[0]) c->clock.add(c->ms[bqsr_compare::BASEQS], bqsr_compare::DECODE1_0, bqsr_compare::DECODE1_1);
  if (c->decoded[1]) c->clock.add(c->ms[bqsr_compare::BASEQS], bqsr_compare::DECODE2_0, bqsr_compare::DECODE2_1);
  for (int side = 0; side < 2; ++side)
    if (h[kCBadUtf + side] != ~0ull) {
      char buf[160];
      snprintf(buf, sizeof buf, "compare: the QUAL bytes of read %llu of input %d are not UTF-8", h[kCBadUtf + side],
               side + 1);
      return fail(BQSR_ERR_SAM_PARSE, buf, (int64_t)h[kCBadUtf + side]);
    }
  // where the reference unboxes a null: positions, mapqs, baseqs; side 1 before side 2
  static const char* const kField[3] = {"start", "mapq", "qual"};
  for (int k = 0; k < 3; ++k)
    for (int side = 0; side < 2; ++side) {
      const cmp_ull r = h[kCNull + 2 * k + side];
      if (r == ~0ull) continue;
      out->null_comparison = kPos + k;
      out->null_side = side + 1;
      out->null_read = (int64_t)r;
      char buf[200];
      snprintf(buf, sizeof buf, "compare: read %llu of input %d has a null %s (the reference throws a "
               "NullPointerException)", r, side + 1, kField[k]);
      return fail(BQSR_ERR_NULL_FIELD, buf, (int64_t)r);
    }
  out->unique1 = (int64_t)h[kCUnique];
  out->unique2 = (int64_t)h[kCUnique + 1];
  out->overmatched[0] = (int64_t)h[kCOver];
  out->overmatched[1] = (int64_t)h[kCOver + 1];
  for (int k = 0; k < 4; ++k) out->dupemismatch[k] = (int64_t)h[kCDupe + k];
  out->flushes = (int32_t)std::min<cmp_ull>(h[kCFlush], INT32_MAX);
  out->n_positions = c->n_pos;
  out->n_mapqs = c->n_mapq;
  out->n_rows = c->n_rows;
  c->ran = true;
  return ok();
}

bqsr_status bqsr_compare_values(const bqsr_compare* c, int32_t comparison, void* values, int64_t* counts) {
  if (!c || !c->ran || (comparison != cmpk::kPos && comparison != cmpk::kMapq))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare_values: bad arguments");
  const int64_t n = comparison == cmpk::kPos ? c->n_pos : c->n_mapq;
  if (n == 0) return ok();
  if (!values || !counts) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare_values: null output");
  HIP_TRY(hipSetDevice(c->ctx->device));
  HIP_TRY(hipMemcpy(values, comparison == cmpk::kPos ? c->pos_val : c->mapq_val, (size_t)n * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(counts, comparison == cmpk::kPos ? c->pos_cnt : c->mapq_cnt, (size_t)n * 8, hipMemcpyDeviceToHost));
  return ok();
}

bqsr_status bqsr_compare_baseqs(const bqsr_compare* c, int64_t* table) {
  if (!c || !c->ran || !table) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare_baseqs: bad arguments");
  HIP_TRY(hipSetDevice(c->ctx->device));
  HIP_TRY(hipMemcpy(table, c->table, (size_t)256 * 256 * 8, hipMemcpyDeviceToHost));
  return ok();
}

bqsr_status bqsr_compare_rows(const bqsr_compare* c, uint32_t* head1, uint32_t* head2) {
  if (!c || !c->ran) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare_rows: bad arguments");
  if (c->n_rows == 0) return ok();
  if (!head1 || !head2) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare_rows: null output");
  HIP_TRY(hipSetDevice(c->ctx->device));
  HIP_TRY(hipMemcpy(head1, c->row1, (size_t)c->n_rows * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(head2, c->row2, (size_t)c->n_rows * 4, hipMemcpyDeviceToHost));
  return ok();
}

bqsr_status bqsr_compare_kernel_times(const bqsr_compare* c, double* join_ms, double* scalar_ms, double* baseqs_ms) {
  if (!c) return fail(BQSR_ERR_INVALID_ARG, "bqsr_compare_kernel_times: null");
  if (join_ms) *join_ms = c->ms[bqsr_compare::JOIN];
  if (scalar_ms) *scalar_ms = c->ms[bqsr_compare::SCALAR];
  if (baseqs_ms) *baseqs_ms = c->ms[bqsr_compare::BASEQS];
  return BQSR_OK;
}

}  // extern "C"
