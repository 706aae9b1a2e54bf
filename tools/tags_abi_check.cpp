// Host-side parts of the print_tags ABI (include/adam_sam.h bqsr_*_tag_*)
// driven without a device: the layout of the structures Python mirrors
// (adam_amd/print_tags.py) and the argument checks every call makes before it
// touches HIP.  Against the built library:
//
//   g++ -std=c++17 -Iinclude tools/tags_abi_check.cpp -Ladam_amd -ladam_bqsr
//       -Wl,-rpath,$PWD/adam_amd -o tags_abi_check && ./tags_abi_check
//
// or, for a sanitizer build of the library's host code, with its sources:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -x hip
//       adam_amd/csrc/bqsr_capi.cpp tools/tags_abi_check.cpp
//       -Xarch_host -fsanitize=address,undefined -o tags_abi_check -lpthread -lz -ldl
//
// Prints a "layout NAME SIZE OFFSET..." line per structure (tests/
// test_tags_abi.py compares them with ctypes), then "tags_abi_check: OK" and
// exit status 0 when every call returned what the header documents.
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

static_assert(sizeof(bqsr_tag_counts) == (128 * 128 + 1) * 8, "bqsr_tag_counts");
static_assert(offsetof(bqsr_tag_counts, total) == 128 * 128 * 8, "bqsr_tag_counts.total");
static_assert(sizeof(bqsr_tags_chunk) == 48, "bqsr_tags_chunk");
static_assert(sizeof(bqsr_tag_value_sizes) == 16, "bqsr_tag_value_sizes");
static_assert(sizeof(bqsr_tag_value_host) == 40, "bqsr_tag_value_host");
static_assert(BQSR_ERR_ATTRIBUTE == 16, "BQSR_ERR_ATTRIBUTE");

int main() {
  std::printf("layout bqsr_tag_counts %zu %zu %zu\n", sizeof(bqsr_tag_counts), offsetof(bqsr_tag_counts, counts),
              offsetof(bqsr_tag_counts, total));
  std::printf("layout bqsr_tags_chunk %zu %zu %zu %zu %zu %zu %zu\n", sizeof(bqsr_tags_chunk),
              offsetof(bqsr_tags_chunk, n_reads), offsetof(bqsr_tags_chunk, attr_offsets),
              offsetof(bqsr_tags_chunk, attr_bytes), offsetof(bqsr_tags_chunk, attr_validity),
              offsetof(bqsr_tags_chunk, failed), offsetof(bqsr_tags_chunk, failed_validity));
  std::printf("layout bqsr_tag_value_sizes %zu %zu %zu\n", sizeof(bqsr_tag_value_sizes),
              offsetof(bqsr_tag_value_sizes, n_runs), offsetof(bqsr_tag_value_sizes, text_bytes));
  std::printf("layout bqsr_tag_value_host %zu %zu %zu %zu %zu %zu\n", sizeof(bqsr_tag_value_host),
              offsetof(bqsr_tag_value_host, type), offsetof(bqsr_tag_value_host, count),
              offsetof(bqsr_tag_value_host, first_read), offsetof(bqsr_tag_value_host, text_offsets),
              offsetof(bqsr_tag_value_host, text));
  if (std::strcmp(bqsr_status_name(BQSR_ERR_ATTRIBUTE), "ATTRIBUTE") != 0) {
    std::fprintf(stderr, "status 16 is named %s\n", bqsr_status_name(BQSR_ERR_ATTRIBUTE));
    ++g_bad;
  }
  // ---- calls refused before any device work
  static bqsr_tag_counts counts;
  std::memset(&counts, 0x5A, sizeof counts);
  bqsr_tags_chunk chunk;
  std::memset(&chunk, 0, sizeof chunk);
  bqsr_tag_value_sizes sizes = {-1, -1};
  expect("sam_tag_counts: nulls", bqsr_sam_tag_counts(nullptr, nullptr, nullptr, &counts), BQSR_ERR_INVALID_ARG);
  expect("arrow_tag_counts: null context", bqsr_arrow_tag_counts(nullptr, &chunk, 1, nullptr, &counts),
         BQSR_ERR_INVALID_ARG);
  expect("arrow_tag_counts: null out", bqsr_arrow_tag_counts(nullptr, &chunk, 1, nullptr, nullptr),
         BQSR_ERR_INVALID_ARG);
  if (counts.total != 0x5A5A5A5A5A5A5A5All) {
    std::fprintf(stderr, "tag_counts: wrote on a refused call\n");
    ++g_bad;
  }
  expect("sam_tag_values: nulls", bqsr_sam_tag_values(nullptr, nullptr, "NM", 64, nullptr, &sizes),
         BQSR_ERR_INVALID_ARG);
  expect("arrow_tag_values: null context", bqsr_arrow_tag_values(nullptr, &chunk, 1, "NM", 64, nullptr, &sizes),
         BQSR_ERR_INVALID_ARG);
  expect("arrow_tag_values: null tag", bqsr_arrow_tag_values(nullptr, &chunk, 1, nullptr, 64, nullptr, &sizes),
         BQSR_ERR_INVALID_ARG);
  if (sizes.n_runs != -1 || sizes.text_bytes != -1) {
    std::fprintf(stderr, "tag_values: wrote on a refused call\n");
    ++g_bad;
  }
  expect("fetch: null", bqsr_tag_values_fetch(nullptr), BQSR_ERR_INVALID_ARG);
  // no values call was made on this thread: no runs, one offset
  int64_t off = -1;
  bqsr_tag_value_host host;
  std::memset(&host, 0, sizeof host);
  expect("fetch: null offsets", bqsr_tag_values_fetch(&host), BQSR_ERR_INVALID_ARG);
  host.text_offsets = &off;
  expect("fetch: no runs", bqsr_tag_values_fetch(&host), BQSR_OK);
  if (off != 0) {
    std::fprintf(stderr, "fetch: text_offsets[0] = %lld\n", (long long)off);
    ++g_bad;
  }
  double ms[2] = {-1.0, -1.0};
  expect("kernel_times", bqsr_tags_kernel_times(&ms[0], &ms[1]), BQSR_OK);
  expect("kernel_times: nulls", bqsr_tags_kernel_times(nullptr, nullptr), BQSR_OK);
  if (ms[0] != 0.0 || ms[1] != 0.0) {
    std::fprintf(stderr, "kernel_times: %g %g before any call\n", ms[0], ms[1]);
    ++g_bad;
  }
  if (g_bad) {
    std::fprintf(stderr, "tags_abi_check: %d failures\n", g_bad);
    return 1;
  }
  std::puts("tags_abi_check: OK");
  return 0;
}
