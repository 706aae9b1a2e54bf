// Host-side parts of the pileup aggregation ABI (include/adam_sam.h
// bqsr_pileup_agg_*) driven without a device: the layout of the structures
// Python mirrors (adam_amd/aggregate_pileups.py) and the argument checks every
// call makes before it touches HIP.  Against the built library:
//
//   g++ -std=c++17 -Iinclude tools/pileup_agg_abi_check.cpp -Ladam_amd -ladam_bqsr
//       -Wl,-rpath,$PWD/adam_amd -o pileup_agg_abi_check && ./pileup_agg_abi_check
//
// Prints a "layout NAME SIZE OFFSET..." line per structure (tests/
// test_pileup_agg_abi.py compares them with ctypes), then
// "pileup_agg_abi_check: OK" and exit status 0 when every call returned what
// the header documents.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "adam_sam.h"

static int g_bad = 0;

static void expect(const char* what, bqsr_status got, bqsr_status want) {
  if (got != want) {
    std::fprintf(stderr, "%s: status %d (%s), expected %d\n", what, (int)got, bqsr_last_error(), (int)want);
    ++g_bad;
  } else if (want != BQSR_OK && !std::strlen(bqsr_last_error())) {
    std::fprintf(stderr, "%s: no error text\n", what);
    ++g_bad;
  }
}

static_assert(sizeof(bqsr_pileup_agg_rows) == 8 + 30 * sizeof(void*), "bqsr_pileup_agg_rows");
static_assert(sizeof(bqsr_pileup_agg_sizes) == 24, "bqsr_pileup_agg_sizes");
static_assert(sizeof(bqsr_pileup_agg_host) == 26 * sizeof(void*), "bqsr_pileup_agg_host");

#define OFF(T, f) std::printf(" %zu", offsetof(T, f));

int main() {
  std::printf("layout bqsr_pileup_agg_rows %zu", sizeof(bqsr_pileup_agg_rows));
#define R(f) OFF(bqsr_pileup_agg_rows, f)
  R(n_rows) R(reference_id) R(position) R(range_offset) R(range_length) R(reference_base) R(read_base)
  R(sanger_quality) R(map_quality) R(num_soft_clipped) R(num_reverse_strand) R(count_at_position) R(read_start)
  R(read_end) R(sample_code) R(rg_code) R(name_code) R(reference_id_valid) R(position_valid) R(range_offset_valid)
  R(range_length_valid) R(reference_base_valid) R(read_base_valid) R(sanger_quality_valid) R(map_quality_valid)
  R(num_soft_clipped_valid) R(num_reverse_strand_valid) R(count_at_position_valid) R(read_start_valid)
  R(read_end_valid) R(sample_code_valid)
#undef R
  std::printf("\nlayout bqsr_pileup_agg_sizes %zu %zu %zu %zu\n", sizeof(bqsr_pileup_agg_sizes),
              offsetof(bqsr_pileup_agg_sizes, n_rows), offsetof(bqsr_pileup_agg_sizes, n_groups),
              offsetof(bqsr_pileup_agg_sizes, bitmap_words));
  std::printf("layout bqsr_pileup_agg_host %zu", sizeof(bqsr_pileup_agg_host));
#define H(f) OFF(bqsr_pileup_agg_host, f)
  H(reference_id) H(position) H(range_offset) H(range_length) H(reference_base) H(read_base) H(sanger_quality)
  H(map_quality) H(num_soft_clipped) H(num_reverse_strand) H(count_at_position) H(read_start) H(read_end)
  H(first_row) H(offsets) H(order) H(names) H(range_offset_valid) H(range_length_valid) H(reference_base_valid)
  H(read_base_valid) H(num_soft_clipped_valid) H(num_reverse_strand_valid) H(read_start_valid) H(read_end_valid)
  H(uniform_rg)
#undef H
  std::printf("\n");
  // ---- calls refused before any device work
  bqsr_pileup_agg* agg = (bqsr_pileup_agg*)(uintptr_t)0x5A;
  expect("create: null context", bqsr_pileup_agg_create(nullptr, &agg), BQSR_ERR_INVALID_ARG);
  if (agg != (bqsr_pileup_agg*)(uintptr_t)0x5A) {
    std::fprintf(stderr, "create: wrote on a refused call\n");
    ++g_bad;
  }
  expect("create: null out", bqsr_pileup_agg_create(nullptr, nullptr), BQSR_ERR_INVALID_ARG);
  bqsr_pileup_agg_destroy(nullptr);
  bqsr_pileup_agg_rows rows;
  std::memset(&rows, 0, sizeof rows);
  expect("add_host: null handle", bqsr_pileup_agg_add_host(nullptr, &rows, nullptr), BQSR_ERR_INVALID_ARG);
  int32_t code = 0;
  expect("sam_add: nulls", bqsr_sam_pileup_agg_add(nullptr, nullptr, nullptr, &code, &code, 0, nullptr),
         BQSR_ERR_INVALID_ARG);
  expect("arrow_add: nulls", bqsr_arrow_pileup_agg_add(nullptr, nullptr, nullptr, &code, &code, 0, nullptr),
         BQSR_ERR_INVALID_ARG);
  bqsr_pileup_agg_sizes sizes = {-1, -1, -1};
  expect("run: null handle", bqsr_pileup_agg_run(nullptr, nullptr, &sizes), BQSR_ERR_INVALID_ARG);
  if (sizes.n_rows != -1 || sizes.n_groups != -1 || sizes.bitmap_words != -1) {
    std::fprintf(stderr, "run: wrote on a refused call\n");
    ++g_bad;
  }
  bqsr_pileup_agg_host host;
  std::memset(&host, 0, sizeof host);
  expect("fetch: null handle", bqsr_pileup_agg_fetch(nullptr, &host, nullptr), BQSR_ERR_INVALID_ARG);
  double ms[4] = {-1.0, -1.0, -1.0, -1.0};
  expect("kernel_times", bqsr_pileup_agg_kernel_times(&ms[0], &ms[1], &ms[2], &ms[3]), BQSR_OK);
  expect("kernel_times: nulls", bqsr_pileup_agg_kernel_times(nullptr, nullptr, nullptr, nullptr), BQSR_OK);
  if (ms[0] != 0.0 || ms[1] != 0.0 || ms[2] != 0.0 || ms[3] != 0.0) {
    std::fprintf(stderr, "kernel_times: %g %g %g %g before any run\n", ms[0], ms[1], ms[2], ms[3]);
    ++g_bad;
  }
  if (g_bad) {
    std::fprintf(stderr, "pileup_agg_abi_check: %d failures\n", g_bad);
    return 1;
  }
  std::puts("pileup_agg_abi_check: OK");
  return 0;
}
