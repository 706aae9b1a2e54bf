// bgzf_deflate.hip -- BGZF members deflated on the device: the other half of
// bgzf_inflate.hip, and what bqsr_bgzf_compress does on host threads.
//
// A byte stream in device memory is cut as the host path cuts it (members of
// 65280 bytes, the last one short, no EOF member); a workgroup of kThreads
// takes a member at a time (a persistent grid, one workgroup a CU: see the
// LDS below) and
//   1. stages its bytes in LDS and computes their CRC32 there (128-byte
//      chunks, combined in GF(2) with bgzf_inflate.hip's crc_mult / crc_x8n);
//   2. goes through it in chunks of kChunk positions.  Per chunk: every
//      position has three candidates: the position before it (distance 1: a
//      run), its bucket's first position of THIS chunk when that is before it
//      (a table of 4-byte hashes filled by atomicMin before the lookups), and
//      its bucket's highest position of the EARLIER chunks (atomicMax of
//      position + 1).  The winner of a bucket is decided by position, never
//      by timing.  Each candidate is extended at most 258 bytes, 4 at a time,
//      the longest wins, the nearer one on a tie.  Then the
//      chunk's positions are inserted, and the greedy parse of the chunk
//      is found without a serial walk: next[i] = i + max(1, len[i]), the
//      positions on the path from the chunk's entry marked by pointer doubling
//      (log2 kChunk rounds), compacted by a workgroup scan into 32-bit tokens
//      in global memory (bgzf_inflate.hip's token format) and counted into the
//      literal/length and distance histograms in LDS;
//   3. builds the code lengths (deflate_codes.h; the sort is a rank sort over
//      the workgroup, the tree a lane for the literal/length code and a lane
//      for the distance code), the code-length code and the 16/17/18 run
//      symbols of the dynamic header, and the exact size of the three forms
//      from the histograms: one dynamic block, one fixed block of the same
//      tokens, one stored block (which also wins a tie: a member DEFLATE would
//      not shrink is stored);
//   4. emits the chosen form: per 512 tokens their bit lengths, a workgroup
//      scan, and every lane ORs its token's bits (at most 48) into the LDS
//      buffer that held the input (zeroed; the input is not needed again);
//   5. writes header, body, CRC32 and ISIZE into the member's 64 KiB slot.
// The members' sizes are scanned and bgzf_pack_kernel packs the slots into one
// contiguous buffer: only that is downloaded.
//
// Every loop is bounded by a constant or by the member's size; no match
// refers to bytes before its own member (the tables are cleared per member).
//
// The member routine is written as phases between workgroup barriers
// (DFL_FOR_T .. DFL_SYNC) with all state that crosses a phase in the Lds
// struct, and every update another lane may see is order-independent (max,
// min, add, or).  So the same source also compiles for the host, where a phase is
// a loop over the lanes: bqsr_bgzf_deflate_host runs it there and gives the
// device's bytes, which lets the whole encoder be tested without a GPU.
//
// Included by bqsr_capi.cpp after bam_out.hip.

#include "deflate_codes.h"

namespace dflk {

constexpr int kThreads = 512;
constexpr int kData = 65280;       // bytes of the stream per member (kBgzfData)
constexpr int kSlot = 65536;       // a member's slot
constexpr int kChunk = 2048;       // positions per matching / parsing round
constexpr int kPer = kChunk / kThreads;
constexpr int kHashBits = 12;
constexpr int kInWords = kSlot / 4 + 8;
constexpr int kLit = 288, kDist = 32;
static_assert(kChunk % kThreads == 0 && kChunk > 258, "a match never jumps over a whole chunk");

struct Lds {
  uint32_t in32[kInWords];          // the member's bytes (zeros behind them); the output's bits from step 4 on
  uint32_t head[1 << kHashBits];    // per bucket: the highest inserted position + 1, 0 none
  uint32_t first[1 << kHashBits];   // per bucket: (31 - chunk) << 16 | the chunk's lowest position (atomicMin: a later chunk wins)
  uint32_t m[kChunk];               // per position of the chunk: len << 16 | distance - 1
  uint16_t jmp[2][kChunk + 2];      // pointer doubling; [cl] is the chunk's exit
  uint8_t mark[kChunk + 8];
  uint32_t scan[kThreads];
  uint32_t wsum[kThreads / 64];
  uint32_t scan_total;
  uint32_t lfreq[kLit], dfreq[kDist], cfreq[20];
  uint8_t llen[kLit], dlen[kDist], clen[20];
  uint16_t lcode[kLit], dcode[kDist], ccode[20];
  uint64_t work[2 * kLit + 2 * kDist];  // sorted keys and tree nodes (literal/length, then distance); a token's bits in step 4
  uint16_t cls[kLit + kDist + 4];       // the header's code-length symbols: symbol | extra value << 8
  uint32_t ncls;
  uint32_t crctab[256];
  uint32_t x2n[20];
  uint32_t nl_used, nd_used;
  uint32_t e_next, form, hdr_bits, body_bits, hlit, hdist, hclen, crc;
};

#if defined(__HIP_DEVICE_COMPILE__)
#define DFL_FOR_T for (int t = (int)threadIdx.x, dfl_once = 1; dfl_once; dfl_once = 0)
#define DFL_SYNC() __syncthreads()
__device__ __forceinline__ void dfl_max(uint32_t* p, uint32_t v) { atomicMax(p, v); }
__device__ __forceinline__ void dfl_min(uint32_t* p, uint32_t v) { atomicMin(p, v); }
__device__ __forceinline__ void dfl_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
__device__ __forceinline__ void dfl_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
#else
#define DFL_FOR_T for (int t = 0; t < kThreads; ++t)
#define DFL_SYNC() ((void)0)
inline void dfl_max(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
inline void dfl_min(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
inline void dfl_add(uint32_t* p, uint32_t v) { *p += v; }
inline void dfl_or(uint32_t* p, uint32_t v) { *p |= v; }
#endif

// S.scan[t] -> its exclusive prefix over the workgroup, S.scan_total the sum.
// Called by every lane between phases (it holds its own barriers).  (L: this
// file's Lds or snappy_pages.hip's, which has the same scan fields.)
template <class L>
__host__ __device__ inline void dfl_scan(L& S) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t v = S.scan[t];
  uint32_t inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == 63) S.wsum[wv] = inc;
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (int q = 0; q < kThreads / 64; ++q) {
    const uint32_t w = S.wsum[q];
    before += q < wv ? w : 0u;
    total += w;
  }
  S.scan[t] = before + inc - v;
  if (t == 0) S.scan_total = total;
  __syncthreads();
#else
  uint32_t run = 0;
  for (int t = 0; t < kThreads; ++t) {
    const uint32_t v = S.scan[t];
    S.scan[t] = run;
    run += v;
  }
  S.scan_total = run;
#endif
}

// the 4 bytes at byte p of the staged member
template <class L>
__host__ __device__ __forceinline__ uint32_t ld4(const L& S, int p) {
  const int i = p >> 2, s = (p & 3) * 8;
  const uint32_t a = S.in32[i];
  return s ? (a >> s) | (S.in32[i + 1] << (32 - s)) : a;
}
__host__ __device__ __forceinline__ uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }
__host__ __device__ __forceinline__ int ctz32(uint32_t x) { return __builtin_ctz(x); }  // x != 0
// bytes in[p ..] and in[q ..] have in common, at most maxlen (<= 258), q < p
template <class L>
__host__ __device__ __forceinline__ int extend(const L& S, int p, int q, int maxlen) {
  int l = 0;
  for (int it = 0; it < 65 && l < maxlen; ++it) {
    const uint32_t x = ld4(S, p + l) ^ ld4(S, q + l);
    if (x) {
      l += ctz32(x) >> 3;
      break;
    }
    l += 4;
  }
  return l < maxlen ? l : maxlen;
}
// v's low nb bits (nb <= 48) ORed into the output at bit position bp
__host__ __device__ __forceinline__ void put_bits(Lds& S, uint32_t bp, uint64_t v, int nb) {
  if (nb <= 0) return;
  const uint32_t w = bp >> 5, s = bp & 31u;
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  const uint32_t w0 = lo << s;
  const uint32_t w1 = (s ? lo >> (32 - s) : 0u) | (hi << s);
  const uint32_t w2 = s ? hi >> (32 - s) : 0u;
  if (w0 && w < (uint32_t)kInWords) dfl_or(&S.in32[w], w0);
  if (w1 && w + 1 < (uint32_t)kInWords) dfl_or(&S.in32[w + 1], w1);
  if (w2 && w + 2 < (uint32_t)kInWords) dfl_or(&S.in32[w + 2], w2);
}

// the order the code-length code's lengths are sent in (§3.2.7)
__host__ __device__ inline int cl_ord(int i) {
  const uint8_t o[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return o[i];
}

// One lane: the dynamic header's plan (S.llen / S.dlen hold the dynamic
// lengths), the three forms' sizes, the choice, the chosen form's codes.
__host__ __device__ inline void plan_block(Lds& S, int n) {
  int hlit = 286, hdist = 30;
  while (hlit > 257 && S.llen[hlit - 1] == 0) --hlit;
  while (hdist > 1 && S.dlen[hdist - 1] == 0) --hdist;
  const int N = hlit + hdist;
  auto L = [&](int i) -> int { return i < hlit ? S.llen[i] : S.dlen[i - hlit]; };
  for (int s = 0; s < 20; ++s) S.cfreq[s] = 0;
  int nc = 0;
  auto emit = [&](int sym, int extra) {
    if (nc < kLit + kDist + 4) S.cls[nc++] = (uint16_t)(sym | (extra << 8));
    S.cfreq[sym]++;
  };
  for (int i = 0; i < N;) {  // (every step advances i: at most N steps)
    const int v = L(i);
    int run = 1;
    while (i + run < N && run < 138 && L(i + run) == v) ++run;
    if (v == 0) {
      if (run >= 11) emit(18, run - 11), i += run;
      else if (run >= 3) emit(17, run - 3), i += run;
      else emit(0, 0), i += 1;
    } else {
      emit(v, 0);
      i += 1;
      run -= 1;
      if (run > 6) run = 6;
      if (run >= 3) emit(16, run - 3), i += run;
    }
  }
  S.ncls = (uint32_t)nc;
  // a complete code-length code needs two used symbols
  int used = 0;
  for (int s = 0; s < 19; ++s) used += S.cfreq[s] != 0;
  for (int s = 0; s < 19 && used < 2; ++s)
    if (S.cfreq[s] == 0) S.cfreq[s] = 1, ++used;
  dflc::code_lengths(S.cfreq, 19, 7, S.clen, S.work);
  int hclen = 19;
  while (hclen > 4 && S.clen[cl_ord(hclen - 1)] == 0) --hclen;
  uint32_t hdr = 14 + 3 * (uint32_t)hclen;
  for (int k = 0; k < nc; ++k) {
    const int sym = S.cls[k] & 31;
    hdr += S.clen[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
  }
  // the bodies: the tokens' bits under the dynamic and the fixed codes, from the histograms
  uint32_t dyn = 3 + hdr, fix = 3;
  for (int s = 0; s < 286; ++s) {
    const uint32_t f = S.lfreq[s];
    if (!f) continue;
    const int x = s >= 257 ? dflc::len_extra_bits(s - 257) : 0;
    dyn += f * (uint32_t)(S.llen[s] + x);
    fix += f * (uint32_t)((s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8) + x);
  }
  for (int d = 0; d < 30; ++d) {
    const uint32_t f = S.dfreq[d];
    if (!f) continue;
    dyn += f * (uint32_t)(S.dlen[d] + dflc::dist_extra_bits(d));
    fix += f * (uint32_t)(5 + dflc::dist_extra_bits(d));
  }
  const uint32_t dyn_bytes = (dyn + 7) >> 3, fix_bytes = (fix + 7) >> 3, stored = 5u + (uint32_t)n;
  uint32_t form = dyn_bytes <= fix_bytes ? 2u : 1u;
  if ((form == 2 ? dyn_bytes : fix_bytes) >= stored) form = 0;
  S.form = form;
  S.hlit = (uint32_t)hlit;
  S.hdist = (uint32_t)hdist;
  S.hclen = (uint32_t)hclen;
  if (form == 1) {
    for (int s = 0; s < kLit; ++s) S.llen[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (int d = 0; d < kDist; ++d) S.dlen[d] = 5;
  }
  if (form) {
    dflc::assign_codes(S.llen, kLit, S.lcode);
    dflc::assign_codes(S.dlen, kDist, S.dcode);
    if (form == 2) dflc::assign_codes(S.clen, 19, S.ccode);
  }
}

// One lane: BFINAL, BTYPE and (dynamic) the code lengths into the zeroed output.
__host__ __device__ inline void put_header(Lds& S) {
  uint32_t bp = 0;
  auto put = [&](uint32_t v, int nb) {
    put_bits(S, bp, v, nb);
    bp += (uint32_t)nb;
  };
  put(1, 1);
  put(S.form, 2);  // 1 fixed, 2 dynamic
  if (S.form == 2) {
    put(S.hlit - 257, 5);
    put(S.hdist - 1, 5);
    put(S.hclen - 4, 4);
    for (uint32_t i = 0; i < S.hclen && i < 19; ++i) put(S.clen[cl_ord((int)i)], 3);
    for (uint32_t k = 0; k < S.ncls; ++k) {
      const int sym = S.cls[k] & 31, x = S.cls[k] >> 8;
      put(S.ccode[sym], S.clen[sym]);
      if (sym >= 16) put((uint32_t)x, sym == 16 ? 2 : sym == 17 ? 3 : 7);
    }
  }
  S.hdr_bits = bp;
}

// One member: gin[0, n) (1 <= n <= kData, gin 4-byte aligned on the device)
// into slot (kSlot bytes), its size into *size.  gtok: kData words of scratch.
__host__ __device__ inline void deflate_member(Lds& S, const uint8_t* gin, int n, uint32_t* gtok, uint8_t* slot,
                                               uint64_t* size) {
  const uint8_t* in8 = (const uint8_t*)S.in32;
  // ---- 1. the bytes into LDS, the tables cleared, the CRC32 ----
  DFL_FOR_T {
    const int full = n >> 2;
    for (int i = t; i < kInWords; i += kThreads) {
      uint32_t v = 0;
      if (i < full) {
#if defined(__HIP_DEVICE_COMPILE__)
        v = ((const uint32_t*)gin)[i];
#else
        memcpy(&v, gin + 4 * (size_t)i, 4);
#endif
      } else if (i == full) {
        for (int k = 0; k < (n & 3); ++k) v |= (uint32_t)gin[4 * i + k] << (8 * k);
      }
      S.in32[i] = v;
    }
    for (int i = t; i < (1 << kHashBits); i += kThreads) S.head[i] = 0, S.first[i] = 0xFFFFFFFFu;
    if (t < kLit) S.lfreq[t] = 0, S.llen[t] = 0;
    if (t < kDist) S.dfreq[t] = 0, S.dlen[t] = 0;
    if (t < 256) {
      uint32_t c = (uint32_t)t;
      for (int k = 0; k < 8; ++k) c = (c & 1u) ? bgzfk::kCrcPoly ^ (c >> 1) : c >> 1;
      S.crctab[t] = c;
    }
    if (t == 0) {
      S.x2n[0] = 1u << 23;  // x^8
      for (int k = 1; k < 20; ++k) S.x2n[k] = bgzfk::crc_mult(S.x2n[k - 1], S.x2n[k - 1]);
      S.nl_used = S.nd_used = 0;
    }
  }
  DFL_SYNC();
  DFL_FOR_T {
    const int lo = t * 128, hi = lo + 128 < n ? lo + 128 : n;  // kThreads * 128 >= kData
    uint32_t r = 0;
    if (lo < hi) {
      uint32_t crc = 0xFFFFFFFFu;
      for (int i = lo; i < hi; ++i) crc = S.crctab[(crc ^ in8[i]) & 0xFFu] ^ (crc >> 8);
      r = bgzfk::crc_mult(crc ^ 0xFFFFFFFFu, bgzfk::crc_x8n(S.x2n, (uint32_t)(n - hi)));
    }
    S.scan[t] = r;
  }
  DFL_SYNC();
  DFL_FOR_T {
    if (t == 0) {
      uint32_t c = 0;
      for (int q = 0; q < kThreads; ++q) c ^= S.scan[q];
      S.crc = c;
    }
  }
  DFL_SYNC();
  // ---- 2. matches and the greedy parse, a chunk at a time ----
  int e = 0;           // the parse's next position
  uint32_t ntok = 0;
  for (int c0 = 0; c0 < n; c0 += kChunk) {
    const int cl = n - c0 < kChunk ? n - c0 : kChunk;
    const uint32_t ctag = (uint32_t)(31 - c0 / kChunk) << 16;  // (kData / kChunk < 32)
    DFL_FOR_T {
      for (int i = t; i < cl; i += kThreads)
        if (n - (c0 + i) >= 4) dfl_min(&S.first[hash4(ld4(S, c0 + i))], ctag | (uint32_t)i);
    }
    DFL_SYNC();
    DFL_FOR_T {
      for (int i = t; i < cl; i += kThreads) {
        const int p = c0 + i;
        const int maxlen = n - p < 258 ? n - p : 258;
        int best = 0, bd = 0;
        if (maxlen >= 3 && p >= 1) {  // a run
          const int l = extend(S, p, p - 1, maxlen);
          if (l >= 3) best = l, bd = 1;
        }
        if (maxlen >= 4) {
          const uint32_t h = hash4(ld4(S, p));
          const uint32_t f = S.first[h];  // the bucket's first position of this chunk, when it is before p
          if ((f & 0xFFFF0000u) == ctag && (int)(f & 0xFFFFu) < i && i - (int)(f & 0xFFFFu) > 1) {
            const int l = extend(S, p, c0 + (int)(f & 0xFFFFu), maxlen);
            if (l >= 4 && l > best) best = l, bd = i - (int)(f & 0xFFFFu);
          }
          const uint32_t q1 = S.head[h];
          const int d = p - (int)q1 + 1;
          if (q1 != 0 && d > 1 && d <= 32768) {
            const int l = extend(S, p, p - d, maxlen);
            if (l >= 4 && l > best) best = l, bd = d;
          }
        }
        S.m[i] = ((uint32_t)best << 16) | (uint32_t)(bd ? bd - 1 : 0);
        const int nx = i + (best ? best : 1);
        S.jmp[0][i] = (uint16_t)(nx < cl ? nx : cl);
      }
      if (t == 0) S.jmp[0][cl] = S.jmp[1][cl] = (uint16_t)cl;
    }
    DFL_SYNC();
    DFL_FOR_T {
      for (int i = t; i < cl; i += kThreads) {
        const int p = c0 + i;
        if (n - p >= 4) dfl_max(&S.head[hash4(ld4(S, p))], (uint32_t)p + 1u);
        S.mark[i] = p == e;
      }
    }
    DFL_SYNC();
    // the positions on the path from e: after round r every one within 2^(r+1) steps is marked
    // (a mark set early in a round only adds a position of the same path)
    int cur = 0;
    for (int r = 0; r < 12 && (1 << r) < cl; ++r, cur ^= 1) {
      DFL_FOR_T {
        for (int i = t; i < cl; i += kThreads) {
          const int j = S.jmp[cur][i];  // <= cl
          if (S.mark[i] && j < cl) S.mark[j] = 1;
          S.jmp[cur ^ 1][i] = S.jmp[cur][j];
        }
      }
      DFL_SYNC();
    }
    DFL_FOR_T {
      uint32_t c = 0;
      for (int k = 0; k < kPer; ++k) {
        const int i = t * kPer + k;
        c += i < cl && S.mark[i];
      }
      S.scan[t] = c;
    }
    DFL_SYNC();
    dfl_scan(S);
    DFL_FOR_T {
      uint32_t at = ntok + S.scan[t];
      for (int k = 0; k < kPer; ++k) {
        const int i = t * kPer + k;
        if (i >= cl || !S.mark[i]) continue;
        const uint32_t mm = S.m[i];
        const int len = (int)(mm >> 16);
        uint32_t tok;
        if (len) {
          int ls, lb, lx, ds, db, dx;
          dflc::len_symbol(len, &ls, &lb, &lx);
          dflc::dist_symbol((int)(mm & 0x7FFFu), &ds, &db, &dx);
          tok = 0x80000000u | ((mm & 0x7FFFu) << 9) | (uint32_t)len;
          dfl_add(&S.lfreq[257 + ls], 1);
          dfl_add(&S.dfreq[ds], 1);
        } else {
          tok = in8[c0 + i];
          dfl_add(&S.lfreq[tok], 1);
        }
        if (at < (uint32_t)kData) gtok[at] = tok;
        ++at;
        const int nx = i + (len ? len : 1);
        if (nx >= cl) S.e_next = (uint32_t)(c0 + nx);  // (one position of a path leaves the chunk)
      }
    }
    DFL_SYNC();
    if (S.scan_total) {
      e = (int)S.e_next;
      ntok += S.scan_total;
    }
  }
  if (ntok > (uint32_t)kData) ntok = kData;
  // ---- 3. the codes and the form ----
  DFL_FOR_T {
    if (t == 0) {
      S.lfreq[256] = 1;  // end of block
      // at least two distance codes, as zlib sends them: a complete code whatever the matches
      int used = 0;
      for (int d = 0; d < 30; ++d) used += S.dfreq[d] != 0;
      for (int d = 0; d < 30 && used < 2; ++d)
        if (S.dfreq[d] == 0) S.dfreq[d] = 1, ++used;
    }
  }
  DFL_SYNC();
  DFL_FOR_T {  // the used symbols sorted by (count, symbol): each one's rank
    const bool lit = t < 286, dst = t >= 320 && t < 350;
    if (lit || dst) {
      const uint32_t* fr = lit ? S.lfreq : S.dfreq;
      const int s = lit ? t : t - 320, ns = lit ? 286 : 30;
      const uint32_t f = fr[s];
      if (f) {
        int rank = 0;
        for (int u = 0; u < ns; ++u) {
          const uint32_t g = fr[u];
          rank += g != 0 && (g < f || (g == f && u < s));
        }
        S.work[(lit ? 0 : 2 * kLit) + rank] = ((uint64_t)f << 32) | (uint32_t)s;
        dfl_add(lit ? &S.nl_used : &S.nd_used, 1);
      }
    }
  }
  DFL_SYNC();
  DFL_FOR_T {
    if (t == 0) dflc::code_lengths_sorted(S.work, (int)S.nl_used, 15, S.llen, S.work + kLit);
    if (t == 64) dflc::code_lengths_sorted(S.work + 2 * kLit, (int)S.nd_used, 15, S.dlen, S.work + 2 * kLit + kDist);
  }
  DFL_SYNC();
  DFL_FOR_T {
    if (t == 0) plan_block(S, n);
  }
  DFL_SYNC();
  const uint32_t form = S.form;
  uint32_t body_bytes = 5u + (uint32_t)n;
  if (form) {
    // ---- 4. the bits ----
    DFL_FOR_T {
      for (int i = t; i < kInWords; i += kThreads) S.in32[i] = 0;
    }
    DFL_SYNC();
    DFL_FOR_T {
      if (t == 0) put_header(S);
    }
    DFL_SYNC();
    uint32_t base = S.hdr_bits;
    for (uint32_t g0 = 0; g0 < ntok; g0 += kThreads) {
      DFL_FOR_T {
        const uint32_t j = g0 + (uint32_t)t;
        uint64_t v = 0;
        uint32_t nb = 0;
        if (j < ntok) {
          const uint32_t tok = gtok[j];
          if (tok >> 31) {
            int ls, lb, lx, ds, db, dx;
            dflc::len_symbol((int)(tok & 511u), &ls, &lb, &lx);
            dflc::dist_symbol((int)((tok >> 9) & 0x7FFFu), &ds, &db, &dx);
            const uint32_t ll = S.llen[257 + ls], dl = S.dlen[ds];
            v = (uint64_t)S.lcode[257 + ls] | ((uint64_t)lx << ll) | ((uint64_t)S.dcode[ds] << (ll + lb)) |
                ((uint64_t)dx << (ll + lb + dl));
            nb = ll + (uint32_t)lb + dl + (uint32_t)db;
          } else {
            v = S.lcode[tok & 255u];
            nb = S.llen[tok & 255u];
          }
        }
        S.work[t] = v | ((uint64_t)nb << 48);
        S.scan[t] = nb;
      }
      DFL_SYNC();
      dfl_scan(S);
      DFL_FOR_T {
        const uint64_t w = S.work[t];
        put_bits(S, base + S.scan[t], w & 0xFFFFFFFFFFFFull, (int)(w >> 48));
      }
      DFL_SYNC();
      base += S.scan_total;
    }
    DFL_FOR_T {
      if (t == 0) {
        put_bits(S, base, S.lcode[256], S.llen[256]);
        S.body_bits = base + S.llen[256];
      }
    }
    DFL_SYNC();
    body_bytes = (S.body_bits + 7) >> 3;
    if (body_bytes > (uint32_t)(kSlot - 26)) body_bytes = kSlot - 26;  // (the plan chose a form below 5 + n bytes)
  }
  // ---- 5. the member ----
  DFL_FOR_T {
    uint8_t* body = slot + 18;
    if (form) {
      const uint16_t* o16 = (const uint16_t*)S.in32;
      uint16_t* b16 = (uint16_t*)body;  // (slot + 18: 2-byte aligned)
      for (uint32_t i = (uint32_t)t; i < body_bytes / 2; i += kThreads) b16[i] = o16[i];
      if (t == 0 && (body_bytes & 1u)) body[body_bytes - 1] = in8[body_bytes - 1];
    } else {
      for (int i = t; i < n; i += kThreads) body[5 + i] = in8[i];
    }
    if (t == 0) {
      const uint8_t head[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
      for (int k = 0; k < 16; ++k) slot[k] = head[k];
      const uint32_t sz = 26u + body_bytes;
      slot[16] = (uint8_t)((sz - 1) & 0xFFu);
      slot[17] = (uint8_t)((sz - 1) >> 8);
      if (!form) {  // BFINAL = 1, BTYPE = 00, LEN, ~LEN
        body[0] = 1;
        body[1] = (uint8_t)(n & 0xFF);
        body[2] = (uint8_t)(n >> 8);
        body[3] = (uint8_t)(~n & 0xFF);
        body[4] = (uint8_t)((~n >> 8) & 0xFF);
      }
      uint8_t* tail = body + body_bytes;
      for (int k = 0; k < 4; ++k) tail[k] = (uint8_t)(S.crc >> (8 * k)), tail[4 + k] = (uint8_t)((uint32_t)n >> (8 * k));
      *size = sz;
    }
  }
  DFL_SYNC();
}

extern "C" __global__ void __launch_bounds__(kThreads) bgzf_deflate_kernel(const uint8_t* in, int64_t n, int64_t nm,
                                                                          uint32_t* tok, uint8_t* slots,
                                                                          uint64_t* sizes) {
  __shared__ Lds S;
  for (int64_t m = blockIdx.x; m < nm; m += gridDim.x) {  // (uniform over the workgroup)
    const int64_t left = n - m * kData;
    const int len = (int)(left < kData ? left : kData);
    if (len <= 0) break;
    deflate_member(S, in + m * kData, len, tok + (int64_t)blockIdx.x * kData, slots + m * kSlot, sizes + m);
  }
}

// the slots' members one after another: out + off[m], dwords once the destination is aligned
extern "C" __global__ void __launch_bounds__(256) bgzf_pack_kernel(const uint8_t* slots, const uint64_t* sizes,
                                                                   const uint64_t* off, int64_t nm, uint8_t* out) {
  for (int64_t m = blockIdx.x; m < nm; m += gridDim.x) {
    const uint8_t* src = slots + m * kSlot;
    const uint32_t* s32 = (const uint32_t*)src;
    const int sz = (int)(sizes[m] < (uint64_t)kSlot ? sizes[m] : (uint64_t)kSlot);
    uint8_t* o = out + off[m];
    const int t = threadIdx.x;
    const int a = (int)((4u - ((uintptr_t)o & 3u)) & 3u), head = a < sz ? a : sz;
    if (t < head) o[t] = src[t];
    const int nw = (sz - head) >> 2;
    uint32_t* o32 = (uint32_t*)(o + head);
    for (int i = t; i < nw; i += 256) {
      const int q = head + 4 * i, s = (q & 3) * 8;
      o32[i] = s ? (s32[q >> 2] >> s) | (s32[(q >> 2) + 1] << (32 - s)) : s32[q >> 2];
    }
    for (int i = head + 4 * nw + t; i < sz; i += 256) o[i] = src[i];
  }
}

// the float tags' binary32 values into the record stream (bam_out.hip's patch list)
extern "C" __global__ void bam_float_scatter(uint8_t* out, int64_t total, const uint64_t* patch, const uint32_t* val,
                                             int64_t n) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t at = patch[2 * k];
    if (at + 4 > (uint64_t)total) continue;
    const uint32_t v = val[k];
    for (int b = 0; b < 4; ++b) out[at + b] = (uint8_t)(v >> (8 * b));
  }
}

}  // namespace dflk

namespace {

// the member kernel and the pack kernel of the calling thread's last device deflate, and the clock's marks
enum { DEFLATE_MEMBERS, DEFLATE_PACK, DEFLATE_STAGES };
enum { DEFLATE_MEMBERS_0, DEFLATE_MEMBERS_1, DEFLATE_PACK_0, DEFLATE_PACK_1 };
thread_local double g_deflate_ms[DEFLATE_STAGES] = {0.0, 0.0};

// d_in[0, n) (device memory, 4-byte aligned, readable to n rounded up to 4)
// deflated into members, packed: *d_out (kept in tmp), *total bytes, *nm members
bqsr_status bgzf_deflate_device(bqsr_context* ctx, const uint8_t* d_in, int64_t n, hipStream_t s,
                                std::vector<void*>& tmp, uint8_t** d_out, int64_t* total, int64_t* nm_out) {
  const int64_t nm = (n + dflk::kData - 1) / dflk::kData;
  *nm_out = nm;
  *total = 0;
  *d_out = nullptr;
  g_deflate_ms[DEFLATE_MEMBERS] = g_deflate_ms[DEFLATE_PACK] = 0.0;
  if (nm == 0) return BQSR_OK;
  const unsigned grid = (unsigned)std::min<int64_t>(nm, std::max<int64_t>(1, (int64_t)ctx->n_cu));
  bqsr_status st;
  uint32_t* tok;
  uint8_t* slots;
  uint64_t *sizes, *off, *part;
  if ((st = sam_alloc(tmp, &tok, (size_t)grid * dflk::kData)) != BQSR_OK ||
      (st = sam_alloc(tmp, &slots, (size_t)nm * dflk::kSlot + 64)) != BQSR_OK ||
      (st = sam_alloc(tmp, &sizes, (size_t)nm + 1)) != BQSR_OK || (st = sam_alloc(tmp, &off, (size_t)nm + 1)) != BQSR_OK ||
      (st = sam_alloc(tmp, &part, (size_t)(nm / samk::kScanChunk + 2))) != BQSR_OK)
    return st;
  StageClock<4> clock;
  HIP_TRY(clock.mark(DEFLATE_MEMBERS_0, s));
  JOB_TRY(launch(dflk::bgzf_deflate_kernel, grid, dflk::kThreads, s, d_in, n, nm, tok, slots, sizes));
  HIP_TRY(clock.mark(DEFLATE_MEMBERS_1, s));
  if ((st = sam_scan(sizes, nm, off, part, s)) != BQSR_OK) return st;
  uint64_t tot = 0;
  HIP_TRY(hipMemcpyAsync(&tot, off + nm, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (tot > (uint64_t)nm * dflk::kSlot) return fail(BQSR_ERR_DEVICE, "bgzf deflate: member sizes out of range");
  uint8_t* packed;
  if ((st = sam_alloc(tmp, &packed, (size_t)tot + 64)) != BQSR_OK) return st;
  HIP_TRY(clock.mark(DEFLATE_PACK_0, s));
  JOB_TRY(launch(dflk::bgzf_pack_kernel, (unsigned)std::min<int64_t>(nm, (int64_t)ctx->n_cu * 8), 256, s, slots, sizes,
                 off, nm, packed));
  HIP_TRY(clock.mark(DEFLATE_PACK_1, s));
  HIP_TRY(hipStreamSynchronize(s));
  clock.add(g_deflate_ms[DEFLATE_MEMBERS], DEFLATE_MEMBERS_0, DEFLATE_MEMBERS_1);
  clock.add(g_deflate_ms[DEFLATE_PACK], DEFLATE_PACK_0, DEFLATE_PACK_1);
  *d_out = packed;
  *total = (int64_t)tot;
  return BQSR_OK;
}

}  // namespace

extern "C" {

bqsr_status bqsr_bgzf_deflate(bqsr_context* ctx, const uint8_t* in, int64_t n, void* stream, uint8_t* out, int64_t cap,
                              int64_t* out_len, int64_t* n_members) {
  if (!ctx || n < 0 || (n > 0 && !in) || !out_len || cap < 0 || (cap > 0 && !out))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_bgzf_deflate: bad arguments");
  *out_len = 0;
  if (n_members) *n_members = 0;
  if (n == 0) return ok();
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  std::vector<void*> tmp;
  struct Free {
    std::vector<void*>& v;
    ~Free() {
      for (void* q : v) (void)hipFree(q);
    }
  } free_tmp{tmp};
  bqsr_status st;
  uint8_t *d_in, *d_out;
  if ((st = sam_alloc(tmp, &d_in, (size_t)n + 64)) != BQSR_OK) return st;
  if ((st = upload_staged(ctx, d_in, in, (size_t)n, s)) != BQSR_OK) return st;
  int64_t total = 0, nm = 0;
  if ((st = bgzf_deflate_device(ctx, d_in, n, s, tmp, &d_out, &total, &nm)) != BQSR_OK) return st;
  *out_len = total;
  if (n_members) *n_members = nm;
  if (total > cap) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bgzf_deflate: the output does not fit (see *out_len)");
  if (total > 0) HIP_TRY(hipMemcpy(out, d_out, (size_t)total, hipMemcpyDeviceToHost));
  return ok();
}

bqsr_status bqsr_bgzf_deflate_host(const uint8_t* in, int64_t n, uint8_t* out, int64_t cap, int64_t* out_len,
                                   int64_t* n_members) {
  if (n < 0 || (n > 0 && !in) || !out_len || cap < 0 || (cap > 0 && !out))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_bgzf_deflate_host: bad arguments");
  const int64_t nm = (n + dflk::kData - 1) / dflk::kData;
  *out_len = 0;
  if (n_members) *n_members = nm;
  if (nm == 0) return ok();
  std::unique_ptr<dflk::Lds> S(new (std::nothrow) dflk::Lds);
  std::vector<uint32_t> tok((size_t)dflk::kData);
  std::vector<uint8_t> slot((size_t)dflk::kSlot);
  if (!S) return fail(BQSR_ERR_DEVICE, "bqsr_bgzf_deflate_host: out of host memory");
  int64_t at = 0;
  bool fits = true;
  for (int64_t m = 0; m < nm; ++m) {
    uint64_t size = 0;
    const int64_t a = m * dflk::kData;
    dflk::deflate_member(*S, in + a, (int)std::min<int64_t>(dflk::kData, n - a), tok.data(), slot.data(), &size);
    if (fits && at + (int64_t)size <= cap) memcpy(out + at, slot.data(), (size_t)size);
    else fits = false;
    at += (int64_t)size;
  }
  *out_len = at;
  if (!fits) return fail(BQSR_ERR_INVALID_ARG, "bqsr_bgzf_deflate_host: the output does not fit (see *out_len)");
  return ok();
}

bqsr_status bqsr_sam_bam_members(bqsr_context* ctx, bqsr_sam* s, void* stream, uint8_t* dst, int64_t cap,
                                 int64_t* out_len) {
  if (!ctx || !s || !out_len || cap < 0 || (cap > 0 && !dst))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_bam_members: bad arguments");
  BamBufs* Ap = (BamBufs*)s->bam.get();
  if (!Ap || !Ap->prepared) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_bam_members before bqsr_sam_bam_prepare");
  BamBufs& A = *Ap;
  if (A.text != s->d_text || A.spans != s->line_span) {  // rewritten or sorted since: the sizes are stale
    A.prepared = false;
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_bam_members: the text changed since bqsr_sam_bam_prepare");
  }
  *out_len = 0;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = S(stream);
  bam_write_begin();
  g_deflate_ms[DEFLATE_MEMBERS] = g_deflate_ms[DEFLATE_PACK] = 0.0;
  if (A.total == 0) return ok();
  JOB_TRY(bam_write_pass(ctx, s, A, st));
  std::vector<void*> tmp;
  struct Free {
    std::vector<void*>& v;
    ~Free() {
      for (void* q : v) (void)hipFree(q);
    }
  } free_tmp{tmp};
  bqsr_status rs;
  if (A.n_float > 0) {
    // the float slots: only the patch list and the texts come to the host, the values go back
    std::vector<uint64_t> patch((size_t)A.n_float * 2);
    std::vector<char> blob((size_t)A.blob_bytes + 1, 0);
    HIP_TRY(hipMemcpyAsync(patch.data(), A.patch, patch.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(blob.data(), A.blob, (size_t)A.blob_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint32_t> val((size_t)A.n_float);
    for (int64_t k = 0; k < A.n_float; ++k) {
      const uint64_t at = patch[2 * (size_t)k], bo = patch[2 * (size_t)k + 1];
      if (at + 4 > (uint64_t)A.total || bo >= (uint64_t)A.blob_bytes)
        return fail(BQSR_ERR_DEVICE, "bqsr_sam_bam_members: a float patch outside the stream");
      const float f = strtof(blob.data() + bo, nullptr);
      memcpy(&val[(size_t)k], &f, 4);
    }
    uint32_t* d_val;
    if ((rs = sam_upload(tmp, &d_val, val, st)) != BQSR_OK) return rs;
    JOB_TRY(launch(dflk::bam_float_scatter, sam_grid(A.n_float, 256, ctx->n_cu * 8), 256, st, A.out, A.total, A.patch,
                   d_val, A.n_float));
    HIP_TRY(hipStreamSynchronize(st));  // (val is read by the copy)
  }
  uint8_t* d_out;
  int64_t total = 0, nm = 0;
  if ((rs = bgzf_deflate_device(ctx, A.out, A.total, st, tmp, &d_out, &total, &nm)) != BQSR_OK) return rs;
  bam_write_end(A);
  *out_len = total;
  if (total > cap) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_bam_members: the output does not fit (see *out_len)");
  if (total > 0) HIP_TRY(hipMemcpy(dst, d_out, (size_t)total, hipMemcpyDeviceToHost));
  return ok();
}

bqsr_status bqsr_deflate_code_lengths(const uint32_t* freq, int32_t n_syms, int32_t max_bits, uint8_t* len_out) {
  if (!freq || !len_out || n_syms < 1 || n_syms > 65536 || max_bits < 1 || max_bits > dflc::kMaxBits ||
      (int64_t)n_syms > (int64_t(1) << max_bits))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_deflate_code_lengths: n_syms must be 1 .. 2^max_bits, max_bits 1 .. 15");
  std::vector<uint64_t> work((size_t)n_syms * 2);
  dflc::code_lengths(freq, n_syms, max_bits, len_out, work.data());
  return ok();
}

bqsr_status bqsr_bgzf_deflate_times(double* deflate_ms, double* pack_ms) {
  if (deflate_ms) *deflate_ms = g_deflate_ms[DEFLATE_MEMBERS];
  if (pack_ms) *pack_ms = g_deflate_ms[DEFLATE_PACK];
  return ok();
}

}  // extern "C"
