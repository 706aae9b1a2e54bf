// The host-side helpers of a resident device job: what a command's state
// struct, its buffers, its rocprim calls, its kernel launches, its launch grids
// and its stage times are made from.  A new job starts from here: DevBuf /
// dev_need / dev_prim for memory, launch for every kernel, a StageClock in the
// state struct with an enum of its stages, and on the Python side one `sig`
// table bound with _capi.bind and _capi.stage_times over the stage names.
// Included by bqsr_capi.cpp once, after fail / HIP_TRY, DevBuf and bqsr_context, before
// sam_ingest.hip.  (The one-shot form of dev_prim, with_temp, sits next to
// sam_alloc in sam_ingest.hip.)
#pragma once

// a step of a job that answers with a bqsr_status (HIP_TRY's counterpart; the message is the step's own)
#define JOB_TRY(expr)                  \
  do {                                 \
    const bqsr_status s_ = (expr);     \
    if (s_ != BQSR_OK) return s_;      \
  } while (0)

namespace {

// a kernel launch and what hipGetLastError() says after it; the arguments convert to the kernel's parameter
// types.  For a site that gathers a hipError_t and frees what it holds itself; every other site uses launch.
template <class... P, class... A>
hipError_t launch_err(void (*kernel)(P...), dim3 grid, dim3 threads, hipStream_t s, A&&... args) {
  kernel<<<grid, threads, 0, s>>>(std::forward<A>(args)...);
  return hipGetLastError();
}

// a kernel launch and its check
template <class... P, class... A>
bqsr_status launch(void (*kernel)(P...), dim3 grid, dim3 threads, hipStream_t s, A&&... args) {
  const hipError_t e = launch_err(kernel, grid, threads, s, std::forward<A>(args)...);
  if (e != hipSuccess) return fail(BQSR_ERR_DEVICE, std::string("hipGetLastError() failed: ") + hipGetErrorString(e));
  return BQSR_OK;
}

// N marks on a stream, the time between any two of them added to a stage.  One
// mark may end a stage and start the next.  The events are made at the first
// mark (or by create()) and live as long as the clock, which owns them and is
// not copied.  add() adds: a job zeroes its stages at its start, so a stage
// read once holds that span and one read per chunk (compare's decode passes,
// the Arrow tag calls) holds their sum.
template <int N>
struct StageClock {
  hipEvent_t ev[N] = {};
  StageClock() = default;
  StageClock(const StageClock&) = delete;
  StageClock& operator=(const StageClock&) = delete;
  ~StageClock() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  hipError_t create() {
    for (hipEvent_t& e : ev)
      if (!e) {
        const hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
      }
    return hipSuccess;
  }
  hipError_t mark(int i, hipStream_t s) {
    const hipError_t r = create();
    return r != hipSuccess ? r : hipEventRecord(ev[i], s);
  }
  // after the job's synchronize: the milliseconds from mark a to mark b, added to ms (left alone if the query fails)
  void add(double& ms, int a, int b) const {
    float v = 0.f;
    if (hipEventElapsedTime(&v, ev[a], ev[b]) == hipSuccess) ms += v;
  }
};

// b (a DevBuf, the device buffer that only grows: bqsr_capi.cpp, where the core's batches hold three) grown to
// count elements of T; a job keeps its whole input's rows on the device, so what does not fit is refused,
// naming the job and what the bytes were for
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
