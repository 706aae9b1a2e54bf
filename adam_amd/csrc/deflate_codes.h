// deflate_codes.h -- the Huffman code construction of a DEFLATE block (RFC
// 1951 §3.2.2, §3.2.7), written once for the host and the device: the encoder
// kernel (bgzf_deflate.hip) and bqsr_deflate_code_lengths call the same code,
// so the part most likely to be subtly wrong is tested without a GPU.
//
// Lengths: the used symbols sorted by (count, symbol), the Huffman tree built
// from the sorted list with two queues (the leaves, the internal nodes in the
// order they are made; a leaf goes first on a tie, which gives the shallowest
// of the optimal trees), then the number of codes per length counted from the
// internal nodes' depths alone: the root offers two places at depth 1, every
// other internal node takes a place at its depth and offers two one level
// down.  A node at or below max_bits takes the deepest free place above
// max_bits instead, so the counts always describe a complete code (Kraft sum
// 1) of at most max_bits bits; the longest lengths go to the rarest symbols.
// Where the tree already fits, the counts are the tree's and the cost is
// Huffman's.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFL_HD __host__ __device__
#else
#define DFL_HD
#endif

namespace dflc {

constexpr int kMaxBits = 15;

// keys: (count << 32 | symbol) of the n used symbols, ascending; node: n words
// of work space.  len[symbol] is written for the used symbols only.  Needs
// 1 <= max_bits <= 15 and n <= 2^max_bits.
DFL_HD inline void code_lengths_sorted(const uint64_t* key, int n, int max_bits, uint8_t* len, uint64_t* node) {
  if (n <= 0) return;
  if (n == 1) {
    len[(uint32_t)key[0]] = 1;
    return;
  }
  // the tree: node[e] is internal node e's weight until it gets a parent, then the parent's index
  int i = 0, b = 0, e = 0;  // the next leaf, the next internal node without a parent, the next one to make
  while (e < n - 1) {
    uint64_t w = 0;
    for (int k = 0; k < 2; ++k) {
      const bool leaf = i < n && (b >= e || (key[i] >> 32) <= node[b]);
      if (leaf) {
        w += key[i++] >> 32;
      } else {
        w += node[b];
        node[b++] = (uint64_t)e;
      }
    }
    node[e++] = w;
  }
  // codes per length from the internal nodes' depths (a parent's index is above its children's)
  uint32_t cnt[kMaxBits + 2];
  for (int l = 0; l < kMaxBits + 2; ++l) cnt[l] = 0;
  cnt[1] = 2;
  node[n - 2] = 0;
  for (int k = n - 3; k >= 0; --k) {
    int d = (int)node[node[k]] + 1;
    node[k] = (uint64_t)d;
    if (d >= max_bits) {
      d = max_bits;
      do --d;
      while (d > 0 && cnt[d] == 0);
      if (d == 0) return;  // (n > 2^max_bits: refused by the callers)
    }
    cnt[d]--;
    cnt[d + 1] += 2;
  }
  int at = 0;
  for (int l = max_bits; l >= 1; --l)
    for (uint32_t c = cnt[l]; c > 0 && at < n; --c) len[(uint32_t)key[at++]] = (uint8_t)l;
}

// freq[n_syms] -> len[n_syms] (0 for an unused symbol, 1 for a single used
// one); work: 2 * n_syms words.  The sort is a heapsort of the keys.
DFL_HD inline void code_lengths(const uint32_t* freq, int n_syms, int max_bits, uint8_t* len, uint64_t* work) {
  uint64_t* key = work;
  int n = 0;
  for (int s = 0; s < n_syms; ++s) {
    len[s] = 0;
    if (freq[s]) key[n++] = ((uint64_t)freq[s] << 32) | (uint32_t)s;
  }
  auto sift = [&](int root, int end) {  // key[root .. end) as a max-heap below root
    for (int guard = 0; guard < 32; ++guard) {
      int c = 2 * root + 1;
      if (c >= end) break;
      if (c + 1 < end && key[c + 1] > key[c]) ++c;
      if (key[root] >= key[c]) break;
      const uint64_t x = key[root];
      key[root] = key[c];
      key[c] = x;
      root = c;
    }
  };
  for (int r = n / 2 - 1; r >= 0; --r) sift(r, n);
  for (int end = n - 1; end > 0; --end) {
    const uint64_t x = key[0];
    key[0] = key[end];
    key[end] = x;
    sift(0, end);
  }
  code_lengths_sorted(key, n, max_bits, len, work + n_syms);
}

// the canonical codes of a set of lengths (§3.2.2), each bit-reversed: DEFLATE
// packs a Huffman code starting from its most significant bit
DFL_HD inline void assign_codes(const uint8_t* len, int n_syms, uint16_t* code) {
  uint32_t cnt[kMaxBits + 1], next[kMaxBits + 1];
  for (int l = 0; l <= kMaxBits; ++l) cnt[l] = 0;
  for (int s = 0; s < n_syms; ++s) cnt[len[s] <= kMaxBits ? len[s] : 0]++;
  cnt[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (int l = 1; l <= kMaxBits; ++l) {
    c = (c + cnt[l - 1]) << 1;
    next[l] = c;
  }
  for (int s = 0; s < n_syms; ++s) {
    const int l = len[s];
    code[s] = 0;
    if (l == 0 || l > kMaxBits) continue;
    uint32_t v = next[l]++, r = 0;
    for (int k = 0; k < l; ++k, v >>= 1) r = (r << 1) | (v & 1u);
    code[s] = (uint16_t)r;
  }
}

// length 3..258 -> its code's index 0..28, extra bits and their value (§3.2.5)
DFL_HD inline void len_symbol(int len, int* ls, int* nb, int* xv) {
  const int l = len - 3;
  if (len == 258) {
    *ls = 28, *nb = 0, *xv = 0;
  } else if (l < 8) {
    *ls = l, *nb = 0, *xv = 0;
  } else {
    int lg = 3;
    while ((l >> (lg + 1)) != 0) ++lg;  // floor(log2 l), l < 256
    const int e = lg - 2;
    *ls = 4 * (e + 1) + ((l >> e) & 3);
    *nb = e;
    *xv = l & ((1 << e) - 1);
  }
}
// distance - 1 (0..32767) -> its code 0..29, extra bits and their value
DFL_HD inline void dist_symbol(int d0, int* ds, int* nb, int* xv) {
  if (d0 < 4) {
    *ds = d0, *nb = 0, *xv = 0;
  } else {
    int lg = 2;
    while ((d0 >> (lg + 1)) != 0) ++lg;  // d0 < 32768
    const int e = lg - 1;
    *ds = 2 * (e + 1) + ((d0 >> e) & 1);
    *nb = e;
    *xv = d0 & ((1 << e) - 1);
  }
}
DFL_HD inline int len_extra_bits(int ls) { return (ls < 8 || ls == 28) ? 0 : (ls - 4) >> 2; }
DFL_HD inline int dist_extra_bits(int ds) { return ds < 4 ? 0 : (ds >> 1) - 1; }

}  // namespace dflc
