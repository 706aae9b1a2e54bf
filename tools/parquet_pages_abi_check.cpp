// Host-side parts of the Parquet page encoder's ABI (include/adam_sam.h
// bqsr_parquet_pages_*, bqsr_*_pileup_device_columns, bqsr_*_pileup_read_spans)
// driven without a device: the layout of the structures Python mirrors
// (adam_amd/parquet_pages.py) and the argument checks every call makes before
// it touches HIP.  Against the built library:
//
//   g++ -std=c++17 -Iinclude tools/parquet_pages_abi_check.cpp -Ladam_amd -ladam_bqsr
//       -Wl,-rpath,$PWD/adam_amd -o parquet_pages_abi_check && ./parquet_pages_abi_check
//
// Prints a "layout NAME SIZE OFFSET..." line per structure (tests/
// test_parquet_pages_abi.py compares them with ctypes), then
// "parquet_pages_abi_check: OK" and exit status 0 when every call returned
// what the header documents.
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

static_assert(sizeof(bqsr_parquet_column) == 64, "bqsr_parquet_column");
static_assert(sizeof(bqsr_parquet_page) == 32, "bqsr_parquet_page");
static_assert(sizeof(bqsr_parquet_pages_sizes) == 16, "bqsr_parquet_pages_sizes");
static_assert(BQSR_PARQUET_PLAIN_INT32 == 0 && BQSR_PARQUET_PLAIN_INT64 == 1 && BQSR_PARQUET_DICT_INDEX == 2, "kinds");

#define OFF(T, f) std::printf(" %zu", offsetof(T, f));

int main() {
  std::printf("layout bqsr_parquet_column %zu", sizeof(bqsr_parquet_column));
#define C(f) OFF(bqsr_parquet_column, f)
  C(kind) C(src_width) C(src) C(src_n) C(gather) C(remap) C(remap_n) C(bit_width) C(base) C(validity)
#undef C
  std::printf("\nlayout bqsr_parquet_page %zu", sizeof(bqsr_parquet_page));
#define P(f) OFF(bqsr_parquet_page, f)
  P(offset) P(bytes) P(rows) P(non_nulls)
#undef P
  std::printf("\nlayout bqsr_parquet_pages_sizes %zu %zu %zu\n", sizeof(bqsr_parquet_pages_sizes),
              offsetof(bqsr_parquet_pages_sizes, n_pages), offsetof(bqsr_parquet_pages_sizes, body_bytes));
  // ---- calls refused before any device work
  bqsr_parquet_pages* enc = (bqsr_parquet_pages*)(uintptr_t)0x5A;
  expect("create: null context", bqsr_parquet_pages_create(nullptr, &enc), BQSR_ERR_INVALID_ARG);
  if (enc != (bqsr_parquet_pages*)(uintptr_t)0x5A) {
    std::fprintf(stderr, "create: wrote on a refused call\n");
    ++g_bad;
  }
  bqsr_parquet_pages_destroy(nullptr);
  int32_t src[64] = {0};
  bqsr_parquet_column col;
  std::memset(&col, 0, sizeof col);
  col.kind = BQSR_PARQUET_DICT_INDEX;
  col.src_width = 4;
  col.src = src;
  col.src_n = 64;
  col.bit_width = 3;
  bqsr_parquet_pages_sizes sz = {-1, -1};
  expect("size: null handle", bqsr_parquet_pages_size(nullptr, &col, 64, 128, nullptr, &sz), BQSR_ERR_INVALID_ARG);
  // (the descriptor is checked before the handle is touched)
  expect("size: page_rows not a multiple of 64", bqsr_parquet_pages_size(enc, &col, 64, 100, nullptr, &sz),
         BQSR_ERR_INVALID_ARG);
  expect("size: null column", bqsr_parquet_pages_size(enc, nullptr, 64, 128, nullptr, &sz), BQSR_ERR_INVALID_ARG);
  expect("size: negative rows", bqsr_parquet_pages_size(enc, &col, -1, 128, nullptr, &sz), BQSR_ERR_INVALID_ARG);
  expect("size: source too short", bqsr_parquet_pages_size(enc, &col, 65, 128, nullptr, &sz), BQSR_ERR_INVALID_ARG);
  bqsr_parquet_column bad = col;
  bad.bit_width = 0;
  expect("size: bit width 0", bqsr_parquet_pages_size(enc, &bad, 64, 128, nullptr, &sz), BQSR_ERR_INVALID_ARG);
  bad.bit_width = 33;
  expect("size: bit width 33", bqsr_parquet_pages_size(enc, &bad, 64, 128, nullptr, &sz), BQSR_ERR_INVALID_ARG);
  bad = col;
  bad.kind = 3;
  expect("size: unknown kind", bqsr_parquet_pages_size(enc, &bad, 64, 128, nullptr, &sz), BQSR_ERR_INVALID_ARG);
  bad = col;
  bad.src_width = 2;
  expect("size: source width 2", bqsr_parquet_pages_size(enc, &bad, 64, 128, nullptr, &sz), BQSR_ERR_INVALID_ARG);
  bad.src_width = 8;
  expect("size: int64 indices", bqsr_parquet_pages_size(enc, &bad, 64, 128, nullptr, &sz), BQSR_ERR_INVALID_ARG);
  bad = col;
  bad.kind = BQSR_PARQUET_PLAIN_INT32;
  bad.base = 1;
  expect("size: base on a PLAIN column", bqsr_parquet_pages_size(enc, &bad, 64, 128, nullptr, &sz),
         BQSR_ERR_INVALID_ARG);
  bad = col;
  bad.remap = src;
  expect("size: remap without entries", bqsr_parquet_pages_size(enc, &bad, 64, 128, nullptr, &sz),
         BQSR_ERR_INVALID_ARG);
  if (sz.n_pages != -1 || sz.body_bytes != -1) {
    std::fprintf(stderr, "size: wrote on a refused call\n");
    ++g_bad;
  }
  uint8_t body[8];
  bqsr_parquet_page page;
  expect("emit: null handle", bqsr_parquet_pages_emit(nullptr, body, &page, nullptr), BQSR_ERR_INVALID_ARG);
  int64_t lo = -7, hi = -7, nn = -7;
  expect("minmax: null handle", bqsr_parquet_pages_minmax(nullptr, &col, 64, nullptr, &lo, &hi, &nn),
         BQSR_ERR_INVALID_ARG);
  expect("minmax: null outputs", bqsr_parquet_pages_minmax(enc, &col, 64, nullptr, nullptr, &hi, &nn),
         BQSR_ERR_INVALID_ARG);
  expect("minmax: null column", bqsr_parquet_pages_minmax(enc, nullptr, 64, nullptr, &lo, &hi, &nn),
         BQSR_ERR_INVALID_ARG);
  if (lo != -7 || hi != -7 || nn != -7) {
    std::fprintf(stderr, "minmax: wrote on a refused call\n");
    ++g_bad;
  }
  bqsr_pileup_host cols;
  expect("sam device_columns: nulls", bqsr_sam_pileup_device_columns(nullptr, nullptr, &cols, nullptr),
         BQSR_ERR_INVALID_ARG);
  expect("arrow device_columns: nulls", bqsr_arrow_pileup_device_columns(nullptr, nullptr, &cols, nullptr),
         BQSR_ERR_INVALID_ARG);
  int64_t span[2] = {-7, -7};
  expect("sam read_spans: nulls", bqsr_sam_pileup_read_spans(nullptr, nullptr, &span[0], &span[1], nullptr),
         BQSR_ERR_INVALID_ARG);
  expect("arrow read_spans: nulls", bqsr_arrow_pileup_read_spans(nullptr, nullptr, &span[0], &span[1], nullptr),
         BQSR_ERR_INVALID_ARG);
  if (span[0] != -7 || span[1] != -7) {
    std::fprintf(stderr, "read_spans: wrote on a refused call\n");
    ++g_bad;
  }
  double ms[2] = {-1.0, -1.0};
  expect("kernel_times", bqsr_parquet_pages_kernel_times(&ms[0], &ms[1]), BQSR_OK);
  expect("kernel_times: nulls", bqsr_parquet_pages_kernel_times(nullptr, nullptr), BQSR_OK);
  if (ms[0] != 0.0 || ms[1] != 0.0) {
    std::fprintf(stderr, "kernel_times: %g %g before any run\n", ms[0], ms[1]);
    ++g_bad;
  }
  if (g_bad) {
    std::fprintf(stderr, "parquet_pages_abi_check: %d failures\n", g_bad);
    return 1;
  }
  std::puts("parquet_pages_abi_check: OK");
  return 0;
}
