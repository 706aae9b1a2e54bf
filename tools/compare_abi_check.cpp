// Host-side parts of the compare ABI (include/adam_sam.h bqsr_compare_*) driven
// without a device: option checks, filter terms, and the argument checks every
// call makes before it touches HIP.  Meant for a sanitizer build of the
// library's host code:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -x hip \
//       adam_amd/csrc/bqsr_capi.cpp tools/compare_abi_check.cpp \
//       -Xarch_host -fsanitize=address,undefined -o compare_abi_check -lpthread -lz -ldl
//   ./compare_abi_check
//
// Exit status 0 and "compare_abi_check: OK" when every call returned what the
// header documents.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

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

static bqsr_compare_options good_options() {
  bqsr_compare_options o;
  std::memset(&o, 0, sizeof o);
  o.hash_bits = 64;
  o.comparisons = 1u << 4;
  return o;
}

int main() {
  // ---- options: refused before the context is looked at
  bqsr_compare* c = reinterpret_cast<bqsr_compare*>(uintptr_t(1));
  bqsr_compare_options o = good_options();
  expect("create: null context", bqsr_compare_create(nullptr, &o, &c), BQSR_ERR_INVALID_ARG);
  if (c != nullptr) {
    std::fprintf(stderr, "create: *out not cleared on failure\n");
    ++g_bad;
  }
  expect("create: null out", bqsr_compare_create(nullptr, &o, nullptr), BQSR_ERR_INVALID_ARG);
  expect("create: default options, null context", bqsr_compare_create(nullptr, nullptr, &c), BQSR_ERR_INVALID_ARG);
  struct Case {
    const char* what;
    void (*set)(bqsr_compare_options&);
  };
  const Case cases[] = {
      {"hash_bits -1", [](bqsr_compare_options& x) { x.hash_bits = -1; }},
      {"hash_bits 65", [](bqsr_compare_options& x) { x.hash_bits = 65; }},
      {"utf8_1 2", [](bqsr_compare_options& x) { x.utf8_1 = 2; }},
      {"utf8_2 -1", [](bqsr_compare_options& x) { x.utf8_2 = -1; }},
      {"comparisons 32", [](bqsr_compare_options& x) { x.comparisons = 32; }},
      {"flush_chars -1", [](bqsr_compare_options& x) { x.flush_chars = -1; }},
      {"flush_chars below a chunk", [](bqsr_compare_options& x) { x.flush_chars = 100; }},
      {"flush_chars above the maximum", [](bqsr_compare_options& x) { x.flush_chars = BQSR_COMPARE_MAX_FLUSH_CHARS + 1; }},
      {"baseq_groups -1", [](bqsr_compare_options& x) { x.baseq_groups = -1; }},
      {"reserved 1", [](bqsr_compare_options& x) { x.reserved = 1; }},
  };
  for (const Case& k : cases) {
    o = good_options();
    k.set(o);
    c = reinterpret_cast<bqsr_compare*>(uintptr_t(1));
    expect(k.what, bqsr_compare_create(nullptr, &o, &c), BQSR_ERR_INVALID_ARG);
    if (std::strstr(bqsr_last_error(), "context")) {  // the option must be what was refused
      std::fprintf(stderr, "%s: passed the option checks\n", k.what);
      ++g_bad;
    }
  }
  // ---- filter terms
  const bqsr_compare_term legal[] = {
      {0, 0, 1, 0}, {0, 0, 0, 0},                       // overmatched = true / false
      {2, 0, 0, 0}, {2, 2, -5, 0}, {2, 3, INT64_MAX, 0},  // positions = < >
      {1, 0, 1, 0}, {1, 1, 0, 1},                       // dupemismatch = !=
      {3, 0, 60, 60}, {3, 1, INT32_MIN, INT32_MAX},     // mapqs
      {4, 0, 40, 40}, {4, 1, -95, 127},                 // baseqs
  };
  expect("terms: every legal form", bqsr_compare_check_terms(legal, (int32_t)(sizeof legal / sizeof legal[0])), BQSR_OK);
  expect("terms: none", bqsr_compare_check_terms(nullptr, 0), BQSR_OK);
  const bqsr_compare_term illegal[] = {
      {5, 0, 0, 0},  {-1, 0, 0, 0},                      // no such comparison
      {0, 1, 1, 0},  {0, 2, 1, 0},  {0, 0, 2, 0},        // overmatched != / < / = 2
      {2, 1, 0, 0},                                      // positions != 0
      {1, 2, 0, 0},  {3, 3, 0, 0},  {4, 4, 0, 0},        // points with < / > / an unknown operator
      {3, (int32_t)0x80000000, 0, 0},
      {4, 0, (int64_t)INT32_MAX + 1, 0}, {1, 0, 0, (int64_t)INT32_MIN - 1},
  };
  for (const bqsr_compare_term& t : illegal) expect("terms: an illegal form", bqsr_compare_check_terms(&t, 1), BQSR_ERR_INVALID_ARG);
  std::vector<bqsr_compare_term> many(17, legal[0]);
  expect("terms: 16", bqsr_compare_check_terms(many.data(), 16), BQSR_OK);
  expect("terms: 17", bqsr_compare_check_terms(many.data(), 17), BQSR_ERR_UNSUPPORTED);
  expect("terms: -1", bqsr_compare_check_terms(many.data(), -1), BQSR_ERR_INVALID_ARG);
  expect("terms: null list", bqsr_compare_check_terms(nullptr, 1), BQSR_ERR_INVALID_ARG);
  many[15] = illegal[5];
  expect("terms: the last one illegal", bqsr_compare_check_terms(many.data(), 16), BQSR_ERR_INVALID_ARG);
  // ---- calls refused before any device work
  bqsr_compare_result r;
  std::memset(&r, 0x5A, sizeof r);
  expect("compare_sam: nulls", bqsr_compare_sam(nullptr, nullptr, nullptr, nullptr, 0, nullptr, &r), BQSR_ERR_INVALID_ARG);
  expect("compare_sam: null result", bqsr_compare_sam(nullptr, nullptr, nullptr, legal, 1, nullptr, nullptr), BQSR_ERR_INVALID_ARG);
  int64_t counts[4];
  int64_t values[4];
  uint32_t rows[4];
  expect("values: null handle", bqsr_compare_values(nullptr, 2, values, counts), BQSR_ERR_INVALID_ARG);
  expect("baseqs: null handle", bqsr_compare_baseqs(nullptr, counts), BQSR_ERR_INVALID_ARG);
  expect("rows: null handle", bqsr_compare_rows(nullptr, rows, rows), BQSR_ERR_INVALID_ARG);
  double ms[3] = {-1.0, -1.0, -1.0};
  expect("kernel_times: null handle", bqsr_compare_kernel_times(nullptr, &ms[0], &ms[1], &ms[2]), BQSR_ERR_INVALID_ARG);
  if (ms[0] != -1.0 || ms[1] != -1.0 || ms[2] != -1.0) {
    std::fprintf(stderr, "kernel_times: wrote without a handle\n");
    ++g_bad;
  }
  bqsr_compare_side side;
  std::memset(&side, 0, sizeof side);
  expect("compare_sides: null handle", bqsr_compare_sides(nullptr, &side, &side, nullptr, 0, nullptr, &r), BQSR_ERR_INVALID_ARG);
  expect("compare_sides: null sides", bqsr_compare_sides(nullptr, nullptr, nullptr, nullptr, 0, nullptr, &r), BQSR_ERR_INVALID_ARG);
  bqsr_compare_destroy(nullptr);
  if (g_bad) {
    std::fprintf(stderr, "compare_abi_check: %d failures\n", g_bad);
    return 1;
  }
  std::puts("compare_abi_check: OK");
  return 0;
}
