// Stand-alone driver of the host sampler (csrc/sampler.cpp + csrc/sampler_x86.cpp, or tests/host/no_avx2.cpp in place of the
// latter), built with a sanitizer by tests/test_host_sanitizers_cpu.py.  It reads a case directory (case_io.h), calls the library
// on heap arrays of exactly the documented sizes and compares every output with the expected bytes the test computed with the
// running interpreter's `random` module.  Exit status 0: every case agreed; 1: the first mismatch is named on stderr.
//
//     sampler_driver <case directory>
#include "case_io.h"

#include "../../include/ggad_hip.h"

using namespace host;

namespace {

struct Gen {
  ggad_mt19937 *g;
  explicit Gen(const Case &c, const char *state_key = "state", const char *index_key = "index") {
    g = ggad_mt_new();
    uint32_t *st = load<uint32_t>(c, state_key, 624);
    expect_rc(c, "ggad_mt_set_state", ggad_mt_set_state(g, st, (int32_t)geti(c, index_key)), GGAD_OK);
    std::free(st);
  }
  ~Gen() { ggad_mt_free(g); }
};

// generator state against random.getstate()[1]: 624 words and the index, exact
void expect_state(const Case &c, ggad_mt19937 *g, const std::string &state_key, const std::string &index_key, const std::string &tag = "") {
  uint32_t *st = exact<uint32_t>(624);
  int32_t *ix = exact<int32_t>(1);
  expect_rc(c, "ggad_mt_get_state", ggad_mt_get_state(g, st, ix), GGAD_OK);
  expect_eq(c, state_key.c_str(), st, 624, tag);
  if (*ix != geti(c, index_key.c_str())) fail(c, tag + index_key + ": got " + std::to_string(*ix) + ", expected " + std::to_string((long long)geti(c, index_key.c_str())));
  std::free(st);
  std::free(ix);
}

// ggad_sched_batches: the schedule in n_calls consecutive calls; out_nodes / out_len of every call are allocations of their own
void run_sched(const Case &c) {
  const int64_t n_train = geti(c, "n_train"), n_pool = geti(c, "n_pool");
  const int32_t bs = (int32_t)geti(c, "batch_size"), n_pseudo = (int32_t)geti(c, "n_pseudo"), bpe = (int32_t)geti(c, "batches_per_epoch");
  const int64_t stride = (int64_t)bs + n_pseudo;
  Gen gen(c);
  int64_t *train = load<int64_t>(c, "train", n_train), *pool = load<int64_t>(c, "pool", n_pool);
  int32_t *in_epoch = exact<int32_t>(1);
  *in_epoch = (int32_t)geti(c, "in_epoch");
  const int n_calls = (int)geti(c, "n_calls");
  int64_t total = 0;
  for (int k = 0; k < n_calls; ++k) total += geti(c, ("count" + std::to_string(k)).c_str());
  int64_t *want_nodes = load<int64_t>(c, "out_nodes", total * stride);
  int32_t *want_len = load<int32_t>(c, "out_len", total);
  int64_t done = 0;
  for (int k = 0; k < n_calls; ++k) {
    const std::string ks = std::to_string(k), tag = "call " + ks + ": ";
    const int32_t count = (int32_t)geti(c, ("count" + ks).c_str());
    int64_t *out_nodes = exact_canary<int64_t>(count * stride);       // rows shorter than the stride keep the canary behind out_len[b]
    int32_t *out_len = exact_canary<int32_t>(count);
    expect_rc(c, "ggad_sched_batches", ggad_sched_batches(gen.g, train, n_train, pool, n_pool, bs, n_pseudo, bpe, in_epoch, count, out_nodes, out_len), GGAD_OK);
    for (int64_t i = 0; i < count; ++i)
      if (out_len[i] != want_len[done + i]) fail(c, tag + "out_len[" + std::to_string(i) + "]: got " + std::to_string(out_len[i]) + ", expected " + std::to_string(want_len[done + i]));
    for (int64_t i = 0; i < count * stride; ++i)
      if (out_nodes[i] != want_nodes[done * stride + i])
        fail(c, tag + "out_nodes[" + std::to_string(i) + "] (batch " + std::to_string(i / stride) + "): got " + std::to_string((long long)out_nodes[i]) + ", expected " + std::to_string((long long)want_nodes[done * stride + i]));
    expect_eq(c, ("train" + ks).c_str(), train, n_train, tag);
    expect_eq(c, ("pool" + ks).c_str(), pool, n_pool, tag);
    if (*in_epoch != geti(c, ("in_epoch" + ks).c_str())) fail(c, tag + "in_epoch: got " + std::to_string(*in_epoch) + ", expected " + std::to_string((long long)geti(c, ("in_epoch" + ks).c_str())));
    expect_state(c, gen.g, "state" + ks, "index" + ks, tag);
    done += count;
    std::free(out_nodes);
    std::free(out_len);
  }
  std::free(train); std::free(pool); std::free(in_epoch); std::free(want_nodes); std::free(want_len);
}

// a call ggad_sched_batches answers without touching anything: outputs keep their canary, lists / generator / counter their contents
void run_sched_refused(const Case &c) {
  const int64_t n_train = geti(c, "n_train"), n_pool = geti(c, "n_pool"), n_pool_arg = geti(c, "n_pool_arg", n_pool);
  const int32_t bs = (int32_t)geti(c, "batch_size"), n_pseudo = (int32_t)geti(c, "n_pseudo"), bpe = (int32_t)geti(c, "batches_per_epoch");
  const int32_t count = (int32_t)geti(c, "count"), alloc = (int32_t)geti(c, "alloc_count");
  const int64_t stride = (int64_t)bs + (n_pseudo > 0 ? n_pseudo : 0);
  const int null_arg = (int)geti(c, "null_arg", 0);
  Gen gen(c);
  int64_t *train = load<int64_t>(c, "train", n_train), *pool = load<int64_t>(c, "pool", n_pool);
  int64_t *train0 = clone(train, n_train), *pool0 = clone(pool, n_pool);
  int32_t *in_epoch = exact<int32_t>(1);
  *in_epoch = (int32_t)geti(c, "in_epoch");
  int64_t *out_nodes = exact_canary<int64_t>(alloc * stride);
  int32_t *out_len = exact_canary<int32_t>(alloc);
  const int rc = ggad_sched_batches(null_arg == 1 ? nullptr : gen.g, null_arg == 2 ? nullptr : train, n_train, null_arg == 3 ? nullptr : pool, n_pool_arg, bs,
                                    n_pseudo, bpe, null_arg == 4 ? nullptr : in_epoch, count, null_arg == 5 ? nullptr : out_nodes,
                                    null_arg == 6 ? nullptr : out_len);
  expect_rc(c, "ggad_sched_batches", rc, geti(c, "expect_rc"));
  expect_canary(c, "out_nodes", out_nodes, alloc * stride);
  expect_canary(c, "out_len", out_len, alloc);
  expect_same(c, "train", train, train0, n_train);
  expect_same(c, "pool", pool, pool0, n_pool);
  if (*in_epoch != geti(c, "in_epoch")) fail(c, "in_epoch changed");
  expect_state(c, gen.g, "state", "index");
  std::free(train); std::free(pool); std::free(train0); std::free(pool0); std::free(in_epoch); std::free(out_nodes); std::free(out_len);
}

// random.seed(seed), then `reps` shuffles of one list: ggad_mt_shuffle_i64 (mode 0) or ggad_mt_shuffle_targets + ggad_apply_swaps_i64
void run_shuffle(const Case &c) {
  const int64_t n = geti(c, "n"), reps = geti(c, "reps");
  const uint64_t seed = ((uint64_t)geti(c, "seed_hi") << 32) | (uint64_t)geti(c, "seed_lo");
  ggad_mt19937 *g = ggad_mt_new();
  expect_rc(c, "ggad_mt_seed_u64", ggad_mt_seed_u64(g, seed), GGAD_OK);
  expect_state(c, g, "state_seeded", "index_seeded");
  int64_t *data = load<int64_t>(c, "data", n);
  for (int64_t r = 0; r < reps; ++r) {
    if (geti(c, "mode") == 0) {
      expect_rc(c, "ggad_mt_shuffle_i64", ggad_mt_shuffle_i64(g, data, n), GGAD_OK);
    } else {
      int32_t *targets = exact_canary<int32_t>(n + 16);
      expect_rc(c, "ggad_mt_shuffle_targets", ggad_mt_shuffle_targets(g, n, targets), GGAD_OK);
      expect_rc(c, "ggad_apply_swaps_i64", ggad_apply_swaps_i64(data, n, targets), GGAD_OK);
      std::free(targets);
    }
  }
  expect_eq(c, "data_out", data, n);
  expect_state(c, g, "state_out", "index_out");
  std::free(data);
  ggad_mt_free(g);
}

// set_state / get_state round trip, then `draws` outputs against random.getrandbits(32); indices outside [0, 624] are refused
void run_state(const Case &c) {
  Gen gen(c);
  expect_state(c, gen.g, "state", "index");
  const int64_t draws = geti(c, "draws");
  uint32_t *bits = exact<uint32_t>(draws);
  for (int64_t i = 0; i < draws; ++i) bits[i] = ggad_mt_getrandbits32(gen.g);
  expect_eq(c, "bits", bits, draws);
  expect_state(c, gen.g, "state_out", "index_out");
  uint32_t *st = load<uint32_t>(c, "state", 624);
  expect_rc(c, "ggad_mt_set_state(index 625)", ggad_mt_set_state(gen.g, st, 625), GGAD_E_INVALID);
  expect_rc(c, "ggad_mt_set_state(index -1)", ggad_mt_set_state(gen.g, st, -1), GGAD_E_INVALID);
  expect_rc(c, "ggad_mt_set_state(NULL)", ggad_mt_set_state(gen.g, nullptr, 0), GGAD_E_INVALID);
  expect_state(c, gen.g, "state_out", "index_out");
  std::free(bits);
  std::free(st);
}

void run_pyset(const Case &c) {
  const int64_t n = geti(c, "n"), rc_want = geti(c, "expect_rc");
  int32_t *keys = load<int32_t>(c, "keys", n), *out = exact_canary<int32_t>(n);
  expect_rc(c, "ggad_pyset_order_i32", ggad_pyset_order_i32(keys, n, out), rc_want);
  if (rc_want == GGAD_OK) expect_eq(c, "order", out, n);
  else expect_canary(c, "out", out, n);
  std::free(keys);
  std::free(out);
}

void run_sample_rows(const Case &c) {
  const int64_t n_nodes = geti(c, "n_nodes"), n_nodes_arg = geti(c, "n_nodes_arg", n_nodes), n_rows = geti(c, "n_rows"), nnz = geti(c, "nnz");
  const int64_t rc_want = geti(c, "expect_rc");
  const int32_t k = (int32_t)geti(c, "k"), k_alloc = (int32_t)geti(c, "k_alloc", k), setsize = (int32_t)geti(c, "setsize");
  const int null_arg = (int)geti(c, "null_arg", 0);
  Gen gen(c);
  int32_t *rowptr = load<int32_t>(c, "rowptr", n_nodes + 1), *col = load<int32_t>(c, "col", nnz);
  int64_t *nodes = load<int64_t>(c, "nodes", n_rows);
  int32_t *nbr = exact_canary<int32_t>(n_rows * k_alloc), *cnt = exact_canary<int32_t>(n_rows);
  const int rc = ggad_mt_sample_rows(null_arg == 1 ? nullptr : gen.g, null_arg == 2 ? nullptr : rowptr, col, n_nodes_arg, null_arg == 3 ? nullptr : nodes, n_rows, k,
                                     setsize, null_arg == 4 ? nullptr : nbr, null_arg == 5 ? nullptr : cnt);
  expect_rc(c, "ggad_mt_sample_rows", rc, rc_want);
  if (rc_want == GGAD_OK) {
    expect_eq(c, "nbr", nbr, n_rows * k);
    expect_eq(c, "cnt", cnt, n_rows);
    expect_state(c, gen.g, "state_out", "index_out");
  } else {
    expect_canary(c, "nbr_out", nbr, n_rows * k_alloc);
    expect_canary(c, "cnt_out", cnt, n_rows);
    expect_state(c, gen.g, "state", "index");
  }
  std::free(rowptr); std::free(col); std::free(nodes); std::free(nbr); std::free(cnt);
}

// table_out spans the batches at their stride and ends with the last batch: (num_batches - 1) * stride + b_max * (3 + k) ints
void run_sage_epoch(const Case &c) {
  const int64_t n_train = geti(c, "n_train"), n_pool = geti(c, "n_pool"), n_nodes = geti(c, "n_nodes"), nnz = geti(c, "nnz"), stride = geti(c, "stride");
  const int32_t bs = (int32_t)geti(c, "batch_size"), n_pseudo = (int32_t)geti(c, "n_pseudo"), nb = (int32_t)geti(c, "num_batches");
  const int32_t k = (int32_t)geti(c, "k"), setsize = (int32_t)geti(c, "setsize"), checked = (int32_t)geti(c, "checked");
  const int64_t rc_want = geti(c, "expect_rc"), table_len = geti(c, "table_len"), len_alloc = geti(c, "len_alloc");
  const int null_arg = (int)geti(c, "null_arg", 0);
  Gen gen(c);
  int64_t *train = load<int64_t>(c, "train", n_train), *pool = load<int64_t>(c, "pool", n_pool), *labels = load<int64_t>(c, "labels", n_nodes);
  int64_t *train0 = clone(train, n_train), *pool0 = clone(pool, n_pool);
  int32_t *rowptr = load<int32_t>(c, "rowptr", n_nodes + 1), *col = load<int32_t>(c, "col", nnz);
  int32_t *table = exact_canary<int32_t>(table_len), *len_out = exact_canary<int32_t>(len_alloc);
  const int rc = ggad_sage_sched_epoch(null_arg == 1 ? nullptr : gen.g, train, n_train, pool, n_pool, bs, n_pseudo, nb, null_arg == 2 ? nullptr : rowptr, col, n_nodes,
                                       null_arg == 3 ? nullptr : labels, k, setsize, checked, null_arg == 4 ? nullptr : table, stride,
                                       null_arg == 5 ? nullptr : len_out);
  expect_rc(c, "ggad_sage_sched_epoch", rc, rc_want);
  if (rc_want == GGAD_OK) {
    expect_eq(c, "table", table, table_len);             // the gaps between batches (stride > b_max * (3 + k)) keep the canary
    expect_eq(c, "len_out", len_out, len_alloc);
    expect_eq(c, "train_out", train, n_train);
    expect_eq(c, "pool_out", pool, n_pool);
    expect_state(c, gen.g, "state_out", "index_out");
  } else {
    expect_canary(c, "table_out", table, table_len);
    expect_canary(c, "len_out", len_out, len_alloc);
    expect_same(c, "train", train, train0, n_train);
    expect_same(c, "pool", pool, pool0, n_pool);
    expect_state(c, gen.g, "state", "index");
  }
  std::free(train); std::free(pool); std::free(labels); std::free(train0); std::free(pool0); std::free(rowptr); std::free(col); std::free(table); std::free(len_out);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <case directory>\n", argv[0]); return 2; }
  const std::vector<Case> cases = read_cases(argv[1]);
  for (const Case &c : cases) {
    if (c.op == "sched") run_sched(c);
    else if (c.op == "sched_refused") run_sched_refused(c);
    else if (c.op == "shuffle") run_shuffle(c);
    else if (c.op == "state") run_state(c);
    else if (c.op == "pyset") run_pyset(c);
    else if (c.op == "sample_rows") run_sample_rows(c);
    else if (c.op == "sage_epoch") run_sage_epoch(c);
    else fail(c, "unknown op");
  }
  std::printf("OK %zu cases\n", cases.size());
  return cases.empty() ? 2 : 0;
}
