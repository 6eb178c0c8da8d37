// Stand-alone driver of the host halves of the panel and ring SpMM plans (csrc/spmm_panel_build.cpp, csrc/spmm_ring_build.cpp),
// built with a sanitizer by tests/test_host_sanitizers_cpu.py.  Every case is one call at the C boundary, recorded while
// Csr.panel_plan / Csr.ring_plan / Csr.value_factors built a plan with the production library: the driver repeats the call on heap
// arrays of exactly the documented sizes and requires the production library's output, byte for byte.  It also checks the read-ahead
// region behind the last tile: every slot there names a zero row (the all-zero LDS rows behind the staged operand: panel_rows
// rounded up to even for the panel stream; slots * slot_rows, + 1 for the lane groups that start odd, for the ring stream).
//
//     builder_driver <case directory>
#include <algorithm>

#include "case_io.h"

#include "../../include/ggad_hip.h"

using namespace host;

namespace {

struct Common {
  int64_t n_rows, nnz, n_rounds;
  int32_t skip_diag, n_threads;
  int null_arg;
  int64_t *rowptr;
  int32_t *col, *round_rows, *round_wide;      // round_wide: NULL when the case has none
  explicit Common(const Case &c) {
    n_rows = geti(c, "n_rows"); nnz = geti(c, "nnz"); n_rounds = geti(c, "n_rounds");
    skip_diag = (int32_t)geti(c, "skip_diag"); n_threads = (int32_t)geti(c, "n_threads"); null_arg = (int)geti(c, "null_arg", 0);
    rowptr = load<int64_t>(c, "rowptr", n_rows + 1);
    col = load<int32_t>(c, "col", nnz);
    round_rows = load<int32_t>(c, "round_rows", n_rounds * 8);
    round_wide = has(c, "round_wide") ? load<int32_t>(c, "round_wide", n_rounds) : nullptr;
  }
  ~Common() { std::free(rowptr); std::free(col); std::free(round_rows); std::free(round_wide); }
  template <class T> T *arg(int which, T *p) const { return null_arg == which ? nullptr : p; }
};

void run_panel_count(const Case &c) {
  Common k(c);
  const int32_t panel_rows = (int32_t)geti(c, "panel_rows"), n_panels = (int32_t)geti(c, "n_panels");
  const int64_t n_out = geti(c, "n_out"), rc_want = geti(c, "expect_rc");       // n_rounds * n_panels of the valid call
  int32_t *steps = exact_canary<int32_t>(n_out);
  const int rc = ggad_spmm_panel_count(k.arg(1, k.rowptr), k.arg(2, k.col), (int32_t)geti(c, "n_rounds_arg", k.n_rounds), k.arg(3, k.round_rows), k.round_wide,
                                       k.skip_diag, panel_rows, n_panels, k.arg(4, steps), k.n_threads);
  expect_rc(c, "ggad_spmm_panel_count", rc, rc_want);
  if (rc_want == 0) expect_eq(c, "steps_rc", steps, n_out);
  else expect_canary(c, "steps_rc", steps, n_out);
  std::free(steps);
}

void run_panel_fill(const Case &c) {
  Common k(c);
  const int32_t panel_rows = (int32_t)geti(c, "panel_rows"), n_panels = (int32_t)geti(c, "n_panels"), spare = (int32_t)geti(c, "spare_octs");
  const int64_t total_octs = geti(c, "total_octs"), n_tiles = k.n_rounds * geti(c, "n_panels_alloc", n_panels), rc_want = geti(c, "expect_rc");
  int32_t *steps = load<int32_t>(c, "steps_rc", n_tiles);
  int64_t *tile_oct = load<int64_t>(c, "tile_oct", n_tiles);
  const int64_t n_stream = (total_octs + spare) * 64;
  uint16_t *stream = exact_canary<uint16_t>(n_stream);
  const int rc = ggad_spmm_panel_fill(k.arg(1, k.rowptr), k.arg(2, k.col), (int32_t)k.n_rounds, k.arg(3, k.round_rows), k.round_wide, k.skip_diag, panel_rows, n_panels,
                                      k.arg(4, steps), k.arg(5, tile_oct), k.arg(6, stream), total_octs, spare, k.n_threads);
  expect_rc(c, "ggad_spmm_panel_fill", rc, rc_want);
  if (rc_want == 0) {
    expect_eq(c, "stream", stream, n_stream);
    const uint16_t zero_row = (uint16_t)(panel_rows + (panel_rows & 1));
    for (int64_t i = total_octs * 64; i < n_stream; ++i)
      if (stream[i] != zero_row) fail(c, "spare oct entry " + std::to_string(i) + " is " + std::to_string(stream[i]) + ", not the zero row " + std::to_string(zero_row));
  } else {
    expect_canary(c, "stream", stream, n_stream);
  }
  std::free(steps); std::free(tile_oct); std::free(stream);
}

void run_values_factor(const Case &c) {
  const int64_t n_rows = geti(c, "n_rows"), nnz = geti(c, "nnz");
  const int null_arg = (int)geti(c, "null_arg", 0);
  int64_t *rowptr = load<int64_t>(c, "rowptr", n_rows + 1);
  int32_t *col = load<int32_t>(c, "col", nnz);
  float *val = load<float>(c, "val", nnz);
  double *r = load<double>(c, "r", n_rows), *rtol = load<double>(c, "rtol", 1);
  const int rc = ggad_spmm_panel_values_factor(null_arg == 1 ? nullptr : rowptr, null_arg == 2 ? nullptr : col, null_arg == 3 ? nullptr : val,
                                               null_arg == 4 ? nullptr : r, (int32_t)geti(c, "n_rows_arg", n_rows), *rtol, (int32_t)geti(c, "n_threads"));
  expect_rc(c, "ggad_spmm_panel_values_factor", rc, geti(c, "expect_rc"));
  std::free(rowptr); std::free(col); std::free(val); std::free(r); std::free(rtol);
}

void run_ring_count(const Case &c) {
  Common k(c);
  const int32_t slot_rows = (int32_t)geti(c, "slot_rows"), slots = (int32_t)geti(c, "n_ring_slots"), window = (int32_t)geti(c, "window");
  const int32_t n_phases = (int32_t)geti(c, "n_phases");
  const int64_t n_out = geti(c, "n_out"), rc_want = geti(c, "expect_rc");
  uint16_t *quads = exact_canary<uint16_t>(n_out);
  const int rc = ggad_spmm_ring_count(k.arg(1, k.rowptr), k.arg(2, k.col), (int32_t)geti(c, "n_rounds_arg", k.n_rounds), k.arg(3, k.round_rows), k.round_wide,
                                      k.skip_diag, slot_rows, slots, window, n_phases, k.arg(4, quads), k.n_threads);
  expect_rc(c, "ggad_spmm_ring_count", rc, rc_want);
  if (rc_want == 0) expect_eq(c, "quads_rp", quads, n_out);
  else expect_canary(c, "quads_rp", quads, n_out);
  std::free(quads);
}

void run_ring_fill(const Case &c) {
  Common k(c);
  const int32_t slot_rows = (int32_t)geti(c, "slot_rows"), slots = (int32_t)geti(c, "n_ring_slots"), window = (int32_t)geti(c, "window");
  const int32_t n_phases = (int32_t)geti(c, "n_phases");
  const int64_t n_sb = geti(c, "n_sb"), n_tiles = geti(c, "n_tiles"), rc_want = geti(c, "expect_rc");
  uint16_t *quads = load<uint16_t>(c, "quads_rp", n_tiles);
  int64_t *quad_off = load<int64_t>(c, "quad_off", n_tiles);
  uint16_t *idx = exact_canary<uint16_t>(n_sb * 128);
  const int rc = ggad_spmm_ring_fill(k.arg(1, k.rowptr), k.arg(2, k.col), (int32_t)k.n_rounds, k.arg(3, k.round_rows), k.round_wide, k.skip_diag, slot_rows, slots,
                                     window, n_phases, k.arg(4, quads), k.arg(5, quad_off), k.arg(6, idx), n_sb, k.n_threads);
  expect_rc(c, "ggad_spmm_ring_fill", rc, rc_want);
  if (rc_want == 0) {
    expect_eq(c, "idx", idx, n_sb * 128);
    int64_t end_quad = 0;                                   // the spare super-blocks: everything behind the last tile
    for (int64_t t = 0; t < n_tiles; ++t)
      if (quads[t]) end_quad = std::max<int64_t>(end_quad, quad_off[t] + quads[t]);
    const uint16_t zero_even = (uint16_t)(slot_rows * slots);
    static const bool first_odd[8] = {false, false, true, true, false, false, true, true};
    if ((end_quad + 3) / 4 >= n_sb) fail(c, "no spare super-block behind the last tile");
    for (int64_t i = (end_quad + 3) / 4 * 128; i < n_sb * 128; ++i) {
      const uint16_t want = (uint16_t)(zero_even + (first_odd[(i >> 3) & 7] ? 1 : 0));
      if (idx[i] != want) fail(c, "spare super-block entry " + std::to_string(i) + " is " + std::to_string(idx[i]) + ", not the zero row " + std::to_string(want));
    }
  } else {
    expect_canary(c, "idx", idx, n_sb * 128);
  }
  std::free(quads); std::free(quad_off); std::free(idx);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <case directory>\n", argv[0]); return 2; }
  const std::vector<Case> cases = read_cases(argv[1]);
  for (const Case &c : cases) {
    if (c.op == "panel_count") run_panel_count(c);
    else if (c.op == "panel_fill") run_panel_fill(c);
    else if (c.op == "values_factor") run_values_factor(c);
    else if (c.op == "ring_count") run_ring_count(c);
    else if (c.op == "ring_fill") run_ring_fill(c);
    else fail(c, "unknown op");
  }
  std::printf("OK %zu cases\n", cases.size());
  return cases.empty() ? 2 : 0;
}
