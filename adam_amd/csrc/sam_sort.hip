// transform -sort_reads on the device (include/adam_sam.h: bqsr_sort_order,
// bqsr_sam_sort): adamSortReadsByReferencePosition
// (core/rdd/AdamRDDFunctions.scala:63-93) over ReferencePosition's ordering
// (models/ReferencePosition.scala:73-95,155-166), the last step of
// Transform.run (cli/Transform.scala:89-93).
//
//   sort_classify   one thread per read: the not-mapped bit (for the unmapped
//       reads' ordinals), the first mapped read with a null referenceId /
//       start (the reference's NullPointerException), the first read the
//       packed key cannot order, the largest mapped referenceId and start
//   scan_* (sam_ingest.hip)   exclusive scan of the not-mapped bits
//   sort_keys       the 64-bit key and the iota payload:
//       mapped    (referenceId << sb) | start     sb = bits of the largest start
//       unmapped  (U + 10000 - c) << sb           U = largest mapped referenceId + 1,
//                 c = ordinal mod 10001 (the reference's key is
//                 (Int.MaxValue - c, Long.MaxValue); only its order matters)
//   rocprim::radix_sort_pairs (stable) over the key bits in use
//   sort_lens       sorted position i -> its record's bytes + 1 ('\n'); records
//       longer than kPiece go on a list
//   scan_*          the records' places in the new text
//   sort_gather     the hot path: a wavefront takes 64 consecutive sorted
//       positions (a lane loads each one's source, place and length), then
//       copies the records four at a time, 16 lanes (256 bytes a pass) each:
//       16-byte stores aligned on the destination, the source read as the
//       two aligned 16-byte words around each chunk and shifted in registers
//       (one shift per record); the bytes in front of the first aligned
//       chunk and behind the last go byte by byte.  No load leaves
//       [0, n_text): a chunk whose second aligned word would is read byte by
//       byte.
//   sort_gather_long   the listed long records, cut into kPiece-byte pieces
//       that the waves of a workgroup copy side by side
//
// bqsr_sam_sort then parses the records of the new text with the record
// kernels of sam_ingest.hip (the handle is that of bqsr_sam_parse of the
// sorted text: columns, spans, counts, referenceName order); MarkDuplicates'
// bits are in the text's FLAG fields by then and come back with the parse.
// Peak device memory: twice the text (the old and the new one), plus the new
// parse's columns beside the old ones until the old handle's are released.
//
// Included by bqsr_capi.cpp after adam_out.hip.

namespace sortk {

constexpr int kThreads = 256;
constexpr int64_t kPiece = 4096;                      // bytes of a long record one wave copies at a time
constexpr uint32_t kWrap = 10001;                     // the reference's counter: 1 .. 10000, then 0
constexpr int64_t kMaxRef = 2147483647ll - 10000;     // mapped referenceIds stay below the unmapped keys
constexpr int64_t kMaxStart = 0xFFFFFFFFll;           // start < 2^32 - 1
// the statistics words of sort_classify / sort_lens
enum { kFirstNull = 0, kFirstBad = 1, kMaxRefP1 = 2, kMaxStartW = 3, kLongCount = 4, kStatWords = 8 };

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d);
    v = o > v ? o : v;
  }
  return v;
}

extern "C" __global__ void __launch_bounds__(kThreads) sort_classify(const uint32_t* flags, const int32_t* ref,
                                                                     const int64_t* start, int64_t n, uint64_t* unm,
                                                                     unsigned long long* st) {
  unsigned long long mref = 0, mstart = 0;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t f = flags[r];
    const bool mapped = (f & BQSR_F_MAPPED) != 0;
    unm[r] = mapped ? 0ull : 1ull;
    if (!mapped) continue;
    const int32_t id = ref[r];
    const int64_t p = start[r];
    if (id == -1 || !(f & BQSR_F_HAS_START)) {
      atomicMin(&st[kFirstNull], (unsigned long long)r);
    } else if (id < 0 || id >= kMaxRef || p < 0 || p >= kMaxStart) {
      atomicMin(&st[kFirstBad], (unsigned long long)r);
    } else {
      mref = max(mref, (unsigned long long)id + 1ull);
      mstart = max(mstart, (unsigned long long)p);
    }
  }
  mref = wave_max(mref);
  mstart = wave_max(mstart);
  if ((threadIdx.x & 63) == 0) {
    if (mref) atomicMax(&st[kMaxRefP1], mref);
    if (mstart) atomicMax(&st[kMaxStartW], mstart);
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) sort_keys(const uint32_t* flags, const int32_t* ref,
                                                                 const int64_t* start, const uint64_t* unm_before,
                                                                 int64_t n, uint64_t first_unmapped, int sb,
                                                                 uint64_t* key, uint32_t* idx) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    uint64_t k;
    if (flags[r] & BQSR_F_MAPPED) {
      k = ((uint64_t)(uint32_t)ref[r] << sb) | (uint64_t)start[r];
    } else {  // AdamRDDFunctions.scala:70-82: the 1-based ordinal among the unmapped reads, mod 10001
      const uint32_t c = (uint32_t)((unm_before[r] + 1ull) % kWrap);
      k = (first_unmapped + (uint64_t)(kWrap - 1u - c)) << sb;
    }
    key[r] = k;
    idx[r] = (uint32_t)r;
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) sort_lens(const uint32_t* order, const uint64_t* line_span,
                                                                 int64_t n, uint64_t* len, uint32_t* long_list,
                                                                 unsigned long long* st) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = order[i];
    const uint64_t L = line_span[2 * r + 1] - line_span[2 * r] + 1ull;
    len[i] = L;
    if ((int64_t)L > kPiece) long_list[atomicAdd(&st[kLongCount], 1ull)] = (uint32_t)i;
  }
}

// bytes [so, so + 16) of src for a chunk whose source is not 16-byte aligned:
// lo / hi are the aligned words at (so & ~15) and 16 beyond, m = so & 15
__device__ __forceinline__ uint4 shift16(uint4 lo, uint4 hi, int m) {
  const int q = m >> 2;
  const uint32_t r = (uint32_t)(m & 3);
  uint32_t w0, w1, w2, w3, w4;
  switch (q) {  // (one value per record)
    case 0: w0 = lo.x, w1 = lo.y, w2 = lo.z, w3 = lo.w, w4 = hi.x; break;
    case 1: w0 = lo.y, w1 = lo.z, w2 = lo.w, w3 = hi.x, w4 = hi.y; break;
    case 2: w0 = lo.z, w1 = lo.w, w2 = hi.x, w3 = hi.y, w4 = hi.z; break;
    default: w0 = lo.w, w1 = hi.x, w2 = hi.y, w3 = hi.z, w4 = hi.w; break;
  }
  return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, r), __builtin_amdgcn_alignbyte(w2, w1, r),
                    __builtin_amdgcn_alignbyte(w3, w2, r), __builtin_amdgcn_alignbyte(w4, w3, r));
}

// A group of G lanes (16 or 64; `lane` = the index in the group): src[s, s +
// nb) -> dst[d, d + nb), then '\n' when nl.  src is 16-byte aligned at offset
// 0 and readable in [0, n_src) only.
template <int G>
__device__ __forceinline__ void copy_piece(const uint8_t* __restrict__ src, int64_t n_src,
                                           uint8_t* __restrict__ dst, int64_t s, int64_t d, int64_t nb, bool nl,
                                           int lane) {
  const int64_t total = nb + (nl ? 1 : 0);
  // the bytes in front of the first 16-byte aligned destination address
  int64_t head = (int64_t)((16u - (uint32_t)((uintptr_t)(dst + d) & 15u)) & 15u);
  if (head > total) head = total;
  if (lane < head) dst[d + lane] = lane < nb ? src[s + lane] : (uint8_t)'\n';
  // whole 16-byte chunks of record bytes
  const int64_t n_chunks = nb > head ? (nb - head) >> 4 : 0;
  const int64_t s0 = s + head, d0 = d + head;
  const int m = (int)(s0 & 15);
  for (int64_t c = lane; c < n_chunks; c += G) {
    const int64_t so = s0 + 16 * c;
    uint4 v;
    if (m == 0) {
      v = *(const uint4*)(src + so);
    } else {
      const int64_t a = so & ~(int64_t)15;
      if (a + 32 <= n_src) {
        v = shift16(*(const uint4*)(src + a), *(const uint4*)(src + a + 16), m);
      } else {  // the text ends inside the second aligned word
        uint32_t w[4];
        for (int j = 0; j < 4; ++j)
          w[j] = (uint32_t)src[so + 4 * j] | ((uint32_t)src[so + 4 * j + 1] << 8) |
                 ((uint32_t)src[so + 4 * j + 2] << 16) | ((uint32_t)src[so + 4 * j + 3] << 24);
        v = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
    *(uint4*)(dst + d0 + 16 * c) = v;
  }
  // what is left (fewer than 16 record bytes, and the newline)
  const int64_t t0 = head + 16 * n_chunks;
  const int64_t k = t0 + lane;
  if (k < total) dst[d + k] = k < nb ? src[s + k] : (uint8_t)'\n';
}

// dst: where the records start in the new text (behind the header); off[i]:
// the place of sorted record i there, off[i + 1] - off[i] its bytes with '\n'
extern "C" __global__ void __launch_bounds__(kThreads) sort_gather(const uint8_t* __restrict__ src, int64_t n_src,
                                                                   uint8_t* __restrict__ dst,
                                                                   const uint32_t* __restrict__ order,
                                                                   const uint64_t* __restrict__ line_span,
                                                                   const uint64_t* __restrict__ off, int64_t n) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < n; i0 += stride) {
    const int64_t i = i0 + lane;
    int64_t s = 0, d = 0, L = 0;
    if (i < n) {
      s = (int64_t)line_span[2 * (int64_t)order[i]];
      d = (int64_t)off[i];
      L = (int64_t)off[i + 1] - d;
      if (L > kPiece) L = 0;  // sort_gather_long's
    }
    // four records at a time, 16 lanes (256 bytes a pass) each: the usual
    // line fits one or two passes, and four copies are in flight per wave
    const int cnt = (int)min((int64_t)64, n - i0);
    for (int j0 = 0; j0 < cnt; j0 += 4) {
      const int j = j0 + (lane >> 4);
      const int64_t Lj = __shfl((long long)L, j), sj = __shfl((long long)s, j), dj = __shfl((long long)d, j);
      if (Lj) copy_piece<16>(src, n_src, dst, sj, dj, Lj - 1, true, lane & 15);
    }
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) sort_gather_long(
    const uint8_t* __restrict__ src, int64_t n_src, uint8_t* __restrict__ dst, const uint32_t* __restrict__ order,
    const uint64_t* __restrict__ line_span, const uint64_t* __restrict__ off, const uint32_t* __restrict__ long_list,
    int64_t n_long) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  for (int64_t k = blockIdx.x; k < n_long; k += gridDim.x) {
    const int64_t i = long_list[k];
    const int64_t s = (int64_t)line_span[2 * (int64_t)order[i]];
    const int64_t d = (int64_t)off[i];
    const int64_t L = (int64_t)off[i + 1] - d;  // with the newline
    const int64_t pieces = (L + kPiece - 1) / kPiece;
    for (int64_t p = wave; p < pieces; p += waves) {
      const int64_t t0 = p * kPiece;
      const int64_t tn = min(kPiece, L - t0);
      const bool nl = t0 + tn == L;
      copy_piece<64>(src, n_src, dst, s + t0, d + t0, tn - (nl ? 1 : 0), nl, lane);
    }
  }
}

}  // namespace sortk

namespace {

struct SortTmp {
  std::vector<void*> v;
  ~SortTmp() {
    for (void* q : v) (void)hipFree(q);
  }
};

// order[i] = the input index of the read at sorted position i (device, [n]);
// enqueued on s (the error checks synchronise it once)
bqsr_status sort_order_device(bqsr_context* ctx, int64_t n, const uint32_t* flags, const int32_t* ref,
                              const int64_t* start, uint32_t* order, hipStream_t s) {
  if (n > 0xFFFFFFFFll) return fail(BQSR_ERR_UNSUPPORTED, "sort_reads: more than 2^32 - 1 reads");
  if (n == 0) return BQSR_OK;
  SortTmp T;
  bqsr_status e;
  uint64_t *unm, *before, *part, *key, *key2;
  unsigned long long* st;
  uint32_t* idx;
  const size_t N = (size_t)n;
  if ((e = sam_alloc(T.v, &unm, N)) || (e = sam_alloc(T.v, &before, N + 1)) ||
      (e = sam_alloc(T.v, &part, N / samk::kScanChunk + 2)) || (e = sam_alloc(T.v, &key, N)) ||
      (e = sam_alloc(T.v, &key2, N)) || (e = sam_alloc(T.v, &idx, N)) ||
      (e = sam_alloc(T.v, &st, (size_t)sortk::kStatWords)))
    return e;
  HIP_TRY(hipMemsetAsync(st, 0xFF, 16, s));  // first null, first unsupported: none
  HIP_TRY(hipMemsetAsync(st + 2, 0, (sortk::kStatWords - 2) * 8, s));
  const unsigned g = sam_grid(n, sortk::kThreads, ctx->n_cu * 16);
  JOB_TRY(launch(sortk::sort_classify, g, sortk::kThreads, s, flags, ref, start, n, unm, st));
  if ((e = sam_scan(unm, n, before, part, s)) != BQSR_OK) return e;
  unsigned long long h[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(h, st, sizeof h, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h[sortk::kFirstNull] != ~0ull) {
    char buf[200];
    snprintf(buf, sizeof buf,
             "sort_reads: read %llu is mapped with a null referenceId or start (the reference's "
             "ReferencePosition(read) throws a NullPointerException)",
             h[sortk::kFirstNull]);
    return fail(BQSR_ERR_NULL_FIELD, buf, (int64_t)h[sortk::kFirstNull]);
  }
  if (h[sortk::kFirstBad] != ~0ull) {
    char buf[200];
    snprintf(buf, sizeof buf,
             "sort_reads: read %llu has a negative referenceId or start, a start of 2^32 - 1 or more, or a "
             "referenceId of Int.MaxValue - 10000 or more",
             h[sortk::kFirstBad]);
    return fail(BQSR_ERR_UNSUPPORTED, buf, (int64_t)h[sortk::kFirstBad]);
  }
  const uint64_t first_unmapped = h[sortk::kMaxRefP1];  // just above the largest mapped referenceId
  const int sb = bits_of(h[sortk::kMaxStartW]);
  const int end_bit = std::max(1, sb + bits_of(first_unmapped + sortk::kWrap - 1));
  JOB_TRY(launch(sortk::sort_keys, g, sortk::kThreads, s, flags, ref, start, before, n, first_unmapped, sb, key, idx));
  if ((e = with_temp(T.v, [&](void* t, size_t& b) {
         return rocprim::radix_sort_pairs(t, b, key, key2, idx, order, N, 0, end_bit, s);
       })))
    return e;
  HIP_TRY(hipStreamSynchronize(s));  // (the temporaries go)
  return BQSR_OK;
}

}  // namespace

extern "C" {

bqsr_status bqsr_sort_order(bqsr_context* ctx, int64_t n, const uint32_t* flags, const int32_t* reference_id,
                            const int64_t* start, uint32_t* order, void* stream) {
  if (!ctx || n < 0 || (n > 0 && (!flags || !reference_id || !start || !order)))
    return fail(BQSR_ERR_INVALID_ARG, "bqsr_sort_order: bad arguments");
  HIP_TRY(hipSetDevice(ctx->device));
  const bqsr_status e = sort_order_device(ctx, n, flags, reference_id, start, order, S(stream));
  return e == BQSR_OK ? ok() : e;
}

bqsr_status bqsr_sam_sort(bqsr_context* ctx, bqsr_sam* sm, void* stream) {
  if (!ctx || !sm) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_sort: bad arguments");
  if (sm->adam && ((AdamBufs*)sm->adam)->out_qual)
    return fail(BQSR_ERR_INVALID_ARG,
                "bqsr_sam_sort: a pending bqsr_sam_adam_set_quals refers to the unsorted records (rewrite the text "
                "first)");
  if (((uintptr_t)sm->d_text & 15) != 0) return fail(BQSR_ERR_INVALID_ARG, "bqsr_sam_sort: misaligned text");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  const int64_t n = sm->n_reads;
  SortTmp T;
  bqsr_status e;
  uint32_t *order, *long_list;
  uint64_t *len, *off, *part;
  unsigned long long* st;
  const size_t N = (size_t)n;
  if ((e = sam_alloc(T.v, &order, N)) != BQSR_OK) return e;
  if ((e = sort_order_device(ctx, n, sm->flags, sm->sq_id, sm->start, order, s)) != BQSR_OK) return e;
  // MarkDuplicates' bits into the FLAG fields, unless the text has them
  if (sm->dup_marked && !sm->flag_text_current &&
      (e = bqsr_sam_rewrite_quals(ctx, sm, nullptr, nullptr, nullptr, nullptr, nullptr, 0, stream)) != BQSR_OK)
    return e;
  if ((e = sam_alloc(T.v, &long_list, N)) || (e = sam_alloc(T.v, &len, N)) || (e = sam_alloc(T.v, &off, N + 1)) ||
      (e = sam_alloc(T.v, &part, N / samk::kScanChunk + 2)) || (e = sam_alloc(T.v, &st, (size_t)sortk::kStatWords)))
    return e;
  HIP_TRY(hipMemsetAsync(st, 0, sortk::kStatWords * 8, s));
  const unsigned g = sam_grid(n, sortk::kThreads, ctx->n_cu * 16);
  if (n > 0)
    JOB_TRY(launch(sortk::sort_lens, g, sortk::kThreads, s, order, sm->line_span, n, len, long_list, st));
  if ((e = sam_scan(len, n, off, part, s)) != BQSR_OK) return e;
  uint64_t body = 0;
  unsigned long long n_long = 0;
  if (n > 0) HIP_TRY(hipMemcpyAsync(&body, off + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&n_long, st + sortk::kLongCount, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int64_t total = sm->header + (int64_t)body;
  uint8_t* nt = nullptr;
  HIP_TRY(hipMalloc(&nt, (size_t)total + 64));
  hipError_t he = hipMemsetAsync(nt + total, 0, 64, s);
  if (he == hipSuccess && sm->header > 0)
    he = hipMemcpyAsync(nt, sm->d_text, (size_t)sm->header, hipMemcpyDeviceToDevice, s);
  if (he == hipSuccess && n > 0) {
    // a wavefront per 64 records: whole workgroups of four
    const unsigned gg = sam_grid((n + 63) / 64 * 64, sortk::kThreads, ctx->n_cu * 8);
    he = launch_err(sortk::sort_gather, gg, sortk::kThreads, s, sm->d_text, sm->n_text, nt + sm->header, order,
                    sm->line_span, off, n);
    if (he == hipSuccess && n_long > 0) {
      const unsigned gl = (unsigned)std::min<int64_t>((int64_t)n_long, (int64_t)ctx->n_cu * 8);
      he = launch_err(sortk::sort_gather_long, gl, sortk::kThreads, s, sm->d_text, sm->n_text, nt + sm->header, order,
                      sm->line_span, off, long_list, (int64_t)n_long);
    }
  }
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  if (he != hipSuccess) {
    (void)hipFree(nt);
    return fail(BQSR_ERR_DEVICE, std::string("bqsr_sam_sort: ") + hipGetErrorString(he));
  }
  // the records of the new text through the record parser
  SamHeader H;
  if ((e = parse_sam_header(sm->header_text.data(), (int64_t)sm->header_text.size(), &H)) != BQSR_OK) {
    (void)hipFree(nt);
    return e;
  }
  bqsr_sam* t = nullptr;
  if ((e = sam_parse_device(ctx, H, sm->header_text.data(), nt, total, s, sm->from_bam, &t)) != BQSR_OK)
    return e;  // (the parse owned nt)
  // the new parse's text and columns into the caller's handle; what the
  // handle carries besides (MarkDuplicates' state, the ADAM buffers) stays
  std::swap(sm->d_text, t->d_text);
  std::swap(sm->n_text, t->n_text);
  std::swap(sm->ref_names, t->ref_names);
  std::swap(sm->n_reads, t->n_reads);
  std::swap(sm->seq_bytes, t->seq_bytes);
  std::swap(sm->qual_bytes, t->qual_bytes);
  std::swap(sm->cig_ops, t->cig_ops);
  std::swap(sm->md_bytes, t->md_bytes);
  std::swap(sm->flags, t->flags);
  std::swap(sm->rg_id, t->rg_id);
  std::swap(sm->ref, t->ref);
  std::swap(sm->sq_id, t->sq_id);
  std::swap(sm->raw_flag, t->raw_flag);
  std::swap(sm->start, t->start);
  std::swap(sm->seq_off, t->seq_off);
  std::swap(sm->seq, t->seq);
  std::swap(sm->qual_off, t->qual_off);
  std::swap(sm->qual, t->qual);
  std::swap(sm->cig_off, t->cig_off);
  std::swap(sm->cig, t->cig);
  std::swap(sm->md_off, t->md_off);
  std::swap(sm->md, t->md);
  std::swap(sm->line_span, t->line_span);
  std::swap(sm->qual_span, t->qual_span);
  std::swap(sm->sq_tab, t->sq_tab);
  std::swap(sm->rg_tab, t->rg_tab);
  std::swap(sm->allocs, t->allocs);
  delete t;
  if (sm->adam) ((AdamBufs*)sm->adam)->prepared = false;
  return ok();
}

}  // extern "C"
