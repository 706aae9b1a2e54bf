// The host-side helpers of a resident device job: what a command's state
// struct, its buffers, its rocprim calls and its launch grids are made from.
// A new job starts from here.  Included by bqsr_capi.cpp once, after fail /
// HIP_TRY and bqsr_context, before sam_ingest.hip.  (The one-shot form of
// dev_prim, with_temp, sits next to sam_alloc in sam_ingest.hip.)
#pragma once

namespace {

// a device buffer that only grows
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// b grown to count elements of T; a job keeps its whole input's rows on the
// device, so what does not fit is refused, naming the job and what the bytes were for
template <class T>
bqsr_status dev_need(DevBuf& b, T** p, size_t count, const char* job, const char* what) {
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  if (b.cap < bytes) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    if (hipMalloc(&b.p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      b.p = nullptr;
      return fail(BQSR_ERR_UNSUPPORTED, std::string(job) + ": one input stays resident on the device and this one does "
                                                          "not fit: " + std::to_string(bytes) + " bytes for its " + what);
    }
    b.cap = bytes;
  }
  *p = (T*)b.p;
  return BQSR_OK;
}

// a rocprim call: asked for its workspace size, then run in `temp` grown to it
template <class F>
bqsr_status dev_prim(DevBuf& temp, const char* job, F&& call) {
  size_t tb = 0;
  HIP_TRY(call((void*)nullptr, tb));
  uint8_t* t;
  const bqsr_status e = dev_need(temp, &t, tb, job, "scan and sort workspace");
  if (e != BQSR_OK) return e;
  HIP_TRY(call((void*)t, tb));
  return BQSR_OK;
}

// a parse's slot for a job's state, made at the job's first call
template <class T>
T* job_state(std::shared_ptr<void>& slot) {
  if (!slot) slot = std::shared_ptr<void>(new T, [](void* p) { delete (T*)p; });
  return (T*)slot.get();
}

unsigned sam_grid(int64_t n, int threads, int cap) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + threads - 1) / threads, cap));
}

// a grid over n items for the jobs built on the pileup walk (BQSR_TUNE_PILEUP_GRID caps these grids as it does
// reads2ref's: tests run every loop through many passes)
unsigned pileup_job_grid(const bqsr_context* ctx, int64_t n, int threads) {
  return sam_grid(n, threads, ctx->tune_pileup_grid > 0 ? ctx->tune_pileup_grid : ctx->n_cu * 8);
}

int bits_of(uint64_t v) {
  int b = 0;
  while (v) {
    ++b;
    v >>= 1;
  }
  return b;
}

}  // namespace
