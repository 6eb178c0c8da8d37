"""The host-only translation units of the library -- csrc/sampler.cpp, csrc/sampler_x86.cpp, csrc/spmm_panel_build.cpp,
csrc/spmm_ring_build.cpp (`HOST_ONLY` in ggad_amd/build.py) -- under AddressSanitizer + UndefinedBehaviorSanitizer and under
ThreadSanitizer.

The other tests reach this code through ctypes with numpy buffers that have slack behind them, and on the AVX2 path only.  Here the
sources are compiled with a sanitizer into stand-alone programs (tests/host/*.cpp: own `main`, no HIP runtime, no Python), which call
the library on heap arrays of exactly the documented sizes and compare every output with expected bytes from outside the code
under test:

* sampler: the running interpreter's `random` module (`seed`, `shuffle`, `sample`, `getrandbits`, `getstate`) and `list(set(..))`;
* plan builders: the arguments of every builder call are recorded at the C boundary while `Csr.panel_plan` / `Csr.ring_plan` /
  `Csr.value_factors` build plans with the production library, and replayed; the outputs must be the production library's, byte for
  byte (what a plan must contain stays with tests/test_fullgraph_{panel,ring}_cpu.py).

The sampler runs in two links: with csrc/sampler_x86.cpp, and with tests/host/no_avx2.cpp in its place (the scalar fall-backs).
`ggad_sched_batches` runs once per setting of its thread switches, each in a process of its own.  A driver is a program of its own:
nothing is preloaded into it and no sanitized code is loaded into python.  A sanitizer report, a mismatch or a child that does not
come back within its cap fails the test.
"""
import ctypes
import math
import os
import random
import shutil
import subprocess
import time

import numpy as np
import pytest
import scipy.sparse as sp
import torch

if torch.cuda.is_available():
    pytest.skip("a GPU is visible: the sanitizer runs of the host-only sources belong on the machine without one",
                allow_module_level=True)

from ggad_amd import _lib                                                    # noqa: E402
from ggad_amd.fullgraph import Csr                                           # noqa: E402
from test_fullgraph_panel_cpu import _normalized                             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ggad_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
CHILD_TIMEOUT = 120            # a cap for a lost wake-up of the pipeline (the child would spin for ever), not a measurement

BASE_FLAGS = ["-O1", "-g", "-fno-omit-frame-pointer", "-std=c++17", "-fPIC", "-Wall", "-pthread"]
SANITIZERS = {
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
    "tsan": ["-fsanitize=thread"],
}
RUN_ENV = {
    "asan_ubsan": {"ASAN_OPTIONS": "halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"},
    "tsan": {"TSAN_OPTIONS": "halt_on_error=1"},
}
REPORT_MARKS = ("ERROR: AddressSanitizer", "runtime error:", "WARNING: ThreadSanitizer")
# exits 0 only when the compiler really instrumented it and the runtime starts
PROBE = {
    "asan_ubsan": "#if defined(__SANITIZE_ADDRESS__)\n#define ON 1\n#elif defined(__has_feature)\n#if __has_feature(address_sanitizer)\n"
                  "#define ON 1\n#endif\n#endif\n#ifndef ON\n#define ON 0\n#endif\n"
                  "int main() { int *p = new int[3]; p[2] = ON; int r = p[2] ? 0 : 3; delete[] p; return r; }\n",
    "tsan": "#if defined(__SANITIZE_THREAD__)\n#define ON 1\n#elif defined(__has_feature)\n#if __has_feature(thread_sanitizer)\n"
            "#define ON 1\n#endif\n#endif\n#ifndef ON\n#define ON 0\n#endif\n"
            "#include <thread>\nint main() { int v = 0; std::thread t([&] { v = ON; }); t.join(); return v ? 0 : 3; }\n",
}
SWITCHES = {
    "defaults": {},
    "C1": {"GGAD_SCHED_C": "1"},
    "C4_M1": {"GGAD_SCHED_C": "4", "GGAD_SCHED_M": "1"},
    "M3": {"GGAD_SCHED_M": "3"},
    "PIN0": {"GGAD_SCHED_PIN": "0"},
}
CANARY64 = np.frombuffer(b"\xa5" * 8, dtype=np.int64)[0]
CANARY32 = np.frombuffer(b"\xa5" * 4, dtype=np.int32)[0]
INT32_MAX = 2 ** 31 - 1


# ---- compiling and running the drivers ---------------------------------------------------------------------------------------------

def _compilers():
    """What ggad_amd/build.py compiles the HOST_ONLY files with (`hipcc -x c++`; linked without the HIP runtime), then g++."""
    out = []
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c) and not any(c == o[1] for o in out):
            out.append(("hipcc", c, ["-no-hip-rt"]))
    gxx = shutil.which("g++")
    if gxx:
        out.append(("g++", gxx, []))
    return out


def _child_env(extra):
    """The whole environment of a driver: where programs, libraries and temporary files are found, the locale, and what the test sets
    (sanitizer options, thread switches).  Nothing else of the shell that started pytest reaches a driver -- no sanitizer options of its
    own, no thread switches, nothing to load into the program."""
    env = {k: v for k, v in os.environ.items() if k in ("PATH", "HOME", "TMPDIR", "LANG", "LC_ALL", "LD_LIBRARY_PATH")}
    env.update(extra)
    return env


def _probe(cc, link_flags, san, workdir):
    src, exe = os.path.join(workdir, "probe.cpp"), os.path.join(workdir, "probe")
    with open(src, "w") as fh:
        fh.write(PROBE[san])
    r = subprocess.run([cc] + BASE_FLAGS + SANITIZERS[san] + link_flags + ["-x", "c++", src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        return "does not build: " + r.stderr.strip()[-300:]
    r = subprocess.run([exe], capture_output=True, text=True, env=_child_env(RUN_ENV[san]), timeout=CHILD_TIMEOUT)
    if r.returncode != 0:
        return f"exit status {r.returncode} (3: built without the sanitizer): " + r.stderr.strip()[-300:]
    return None


class Toolchain:
    def __init__(self, san, workdir):
        self.san, self.dir = san, str(workdir)
        why = []
        for name, cc, link_flags in _compilers():
            pdir = os.path.join(self.dir, "probe_" + name)
            os.makedirs(pdir)
            err = _probe(cc, link_flags, san, pdir)
            if err is None:
                self.name, self.cc, self.link_flags = name, cc, link_flags
                break
            why.append(f"{name}: {err}")
        else:
            pytest.skip(f"no compiler here builds and runs a probe program with {' '.join(SANITIZERS[san])} "
                        f"({'; '.join(why) or 'neither hipcc nor g++ found'}): a run without the sanitizer would prove nothing")
        self._objs, self._exes = {}, {}

    def _objects(self, sources):
        procs = []
        for src in sources:
            if src not in self._objs:
                obj = os.path.join(self.dir, os.path.basename(src) + ".o")
                cmd = [self.cc] + BASE_FLAGS + SANITIZERS[self.san] + ["-x", "c++", "-c", src, "-o", obj]
                procs.append((src, obj, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        for src, obj, p in procs:
            out, _ = p.communicate()
            assert p.returncode == 0, f"{self.name} failed on {src}:\n{out[-3000:]}"
            self._objs[src] = obj
        return [self._objs[s] for s in sources]

    def program(self, name, sources):
        if name not in self._exes:
            exe = os.path.join(self.dir, name)
            r = subprocess.run([self.cc] + self.link_flags + ["-pthread"] + SANITIZERS[self.san] + self._objects(sources) + ["-o", exe],
                               capture_output=True, text=True)
            assert r.returncode == 0, f"{self.name} could not link {name}:\n{r.stderr[-3000:]}"
            self._exes[name] = exe
        return self._exes[name]

    def sampler(self, link):
        x86 = os.path.join(CSRC, "sampler_x86.cpp") if link == "avx2" else os.path.join(HOST, "no_avx2.cpp")
        return self.program("sampler_" + link, [os.path.join(CSRC, "sampler.cpp"), x86, os.path.join(HOST, "sampler_driver.cpp")])

    def builder(self):
        return self.program("builder", [os.path.join(CSRC, "spmm_panel_build.cpp"), os.path.join(CSRC, "spmm_ring_build.cpp"),
                                        os.path.join(HOST, "builder_driver.cpp")])

    def run(self, exe, case_dir, n_cases, switches=None):
        env = _child_env({**RUN_ENV[self.san], **(switches or {})})
        t0 = time.perf_counter()
        try:
            r = subprocess.run([exe, case_dir], capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
            pytest.fail(f"{os.path.basename(exe)} [{self.san}] did not return within {CHILD_TIMEOUT} s (a lost wake-up?)\n"
                        + "\n".join(err.splitlines()[:60]))
        dt = time.perf_counter() - t0
        print(f"[host-sanitizers] {self.name} {self.san} {os.path.basename(exe)} {os.path.basename(case_dir)} "
              f"{' '.join(f'{k}={v}' for k, v in (switches or {}).items()) or '-'}: {dt:.1f} s")
        bad = r.returncode != 0 or any(m in r.stderr for m in REPORT_MARKS)
        if bad:
            print("\n".join(r.stderr.splitlines()[:60]))
        assert r.returncode == 0, f"{os.path.basename(exe)} [{self.san}] exit status {r.returncode}"
        for m in REPORT_MARKS:
            assert m not in r.stderr, f"{os.path.basename(exe)} [{self.san}] reported: {m}"
        assert r.stdout.strip() == f"OK {n_cases} cases"


@pytest.fixture(scope="module", params=list(SANITIZERS))
def toolchain(request, tmp_path_factory):
    return Toolchain(request.param, tmp_path_factory.mktemp("host_" + request.param))


# ---- case directories --------------------------------------------------------------------------------------------------------------

class CaseDir:
    """cases.txt + raw little-endian arrays, the format of tests/host/case_io.h."""

    def __init__(self, path):
        self.path = str(path)
        self.lines, self.n = [], 0

    def add(self, name, op, ints, arrays):
        self.lines.append(f"case {name} {op}")
        for k, v in ints.items():
            self.lines.append(f"i {k} {int(v)}")
        for k, (a, dtype) in arrays.items():
            a = np.ascontiguousarray(a, dtype=dtype)
            assert a.dtype.byteorder in "=|<"
            fn = f"c{self.n}_{k}.bin"
            a.tofile(os.path.join(self.path, fn))
            self.lines.append(f"a {k} {fn}")
        self.lines.append("end")
        self.n += 1

    def close(self):
        with open(os.path.join(self.path, "cases.txt"), "w") as fh:
            fh.write("\n".join(self.lines) + "\n")
        return self.path, self.n


def _py_state():
    """(624 words, index) of the interpreter's generator."""
    st = random.getstate()
    assert st[0] == 3
    return np.array(st[1][:624], dtype=np.uint32), int(st[1][624])


def _set_py_state(words, index):
    random.setstate((3, tuple(int(w) for w in words) + (int(index),), None))


# ---- ggad_sched_batches against the loop the header describes ----------------------------------------------------------------------

def _sched_reference(words, index, train, pool, bs, n_pseudo, bpe, in_epoch, cuts):
    """shuffle train at the epoch start, shuffle the pool before every batch, batch = train[i0:i1] ++ pool[:n_pseudo];
    snapshots of both lists, the counter and the generator after every cut.  Unwritten tails of out_nodes rows hold the canary."""
    _set_py_state(words, index)
    train, pool, ie = list(train), list(pool), in_epoch
    stride = bs + n_pseudo
    rows, lens, snaps = [], [], []
    for count in cuts:
        for _ in range(count):
            if ie >= bpe:
                random.shuffle(train)
                ie = 0
            random.shuffle(pool)
            i0 = ie * bs
            batch = train[i0:min(i0 + bs, len(train))] + pool[:n_pseudo]
            ie += 1
            lens.append(len(batch))
            rows.append(batch + [CANARY64] * (stride - len(batch)))
        snaps.append((list(train), list(pool), ie) + _py_state())
    return np.array(rows, dtype=np.int64).reshape(-1), np.array(lens, dtype=np.int32), snaps


# name: (n_train, n_pool, batch_size, n_pseudo, batches_per_epoch, in_epoch at entry, draws before entry (0: index 624), cuts)
SCHED_CONFIGS = {
    # one batch, the generator on a block boundary, the call opens with the epoch shuffle; the cuts (0, 1, 0) put empty calls around it
    "one_batch": (50, 10, 16, 4, 4, 4, 0, (0, 1, 0)),
    # a partial 8-shuffle segment, entered mid-epoch and mid-block
    "seven_mid_epoch": (100, 40, 16, 5, 7, 2, 100, (2, 3, 2)),
    # one full segment with a pool of ONE id: the pool's end state is the state after an odd number of segments
    "eight_pool1": (64, 1, 16, 1, 4, 1, 7, (3, 1, 4)),
    # calls that END on a segment end with composer threads at work (n_pool >= 2): the pool's final state is the buffer the composers
    # left, no trailing partial segment.  One call of 8 (one segment: the odd buffer); 8 / 16 / 8 and all 32 in one call (even buffers)
    "eight_pool40": (100, 40, 16, 5, 4, 1, 50, (3, 1, 4)),
    "segments_8_16_8": (100, 40, 16, 5, 4, 3, 77, (8, 16, 8)),
    "sixteen_pool300": (70, 300, 16, 257, 5, 5, 0, (8, 8, 0)),
    # 129 batches (the 128-slot ring reused once), n_train < batch_size, batches_per_epoch = 1: an epoch shuffle before EVERY batch
    # (the train double buffer reused 64 times), n_pool == n_pseudo == 300
    "ring_once_epoch_each": (40, 300, 64, 300, 1, 1, 623, (50, 60, 19)),
    # 300 batches in one call (the ring reused twice), three epoch shuffles inside it, 20,000-id pool: ~ 8 M generator outputs wrap the
    # 256-block ring 50 times; n_pseudo = 257 = one whole 256-block of chain look-ups and one more
    "ring_twice_big": (55000, 20000, 128, 257, 100, 100, 311, (100, 129, 71)),
    # no pool at all, more batches than ring slots
    "pool0_130": (200, 0, 32, 0, 7, 3, 5, (1, 128, 1)),
    # a pool of one id across the ring reuse, 17 full segments
    "pool1_137": (90, 1, 16, 1, 6, 0, 9, (64, 65, 8)),
    # a pool of two; batches 2 and 3 of an epoch start behind the end of train (i0 >= n_train): pseudo rows only
    "pool2_past_train": (30, 2, 16, 1, 4, 0, 333, (6, 7, 7)),
    # n_pseudo = 256 exactly; entered with in_epoch far beyond batches_per_epoch
    "pseudo256": (77, 1000, 10, 256, 3, 99, 12, (4, 4, 1)),
    # a pool that is shuffled but never read
    "pseudo0": (64, 50, 8, 0, 8, 8, 624 + 17, (5, 5, 7)),
}


def _sched_cases(path):
    cd = CaseDir(path)
    for name, (n_train, n_pool, bs, n_pseudo, bpe, in_epoch, draws, cuts) in SCHED_CONFIGS.items():
        random.seed(sum(map(ord, name)))
        for _ in range(draws):
            random.getrandbits(32)
        words, index = _py_state()
        assert (index == 624) == (draws == 0)
        train = [1000 + 3 * i for i in range(n_train)]
        pool = [INT32_MAX - 7 * i for i in range(n_pool)]                   # pool ids are int32 inside the pipeline: the top of the range
        nodes, lens, snaps = _sched_reference(words, index, train, pool, bs, n_pseudo, bpe, in_epoch, cuts)
        base_i = dict(n_train=n_train, n_pool=n_pool, batch_size=bs, n_pseudo=n_pseudo, batches_per_epoch=bpe, in_epoch=in_epoch, index=index)
        base_a = dict(train=(train, np.int64), pool=(pool, np.int64), state=(words, np.uint32), out_nodes=(nodes, np.int64), out_len=(lens, np.int32))
        for label, calls, which in (("one_call", (sum(cuts),), (len(cuts) - 1,)), ("three_calls", cuts, range(len(cuts)))):
            ints, arrays = dict(base_i, n_calls=len(calls)), dict(base_a)
            for k, (count, s) in enumerate(zip(calls, which)):
                tr, po, ie, w, ix = snaps[s]
                ints.update({f"count{k}": count, f"in_epoch{k}": ie, f"index{k}": ix})
                arrays.update({f"train{k}": (tr, np.int64), f"pool{k}": (po, np.int64), f"state{k}": (w, np.uint32)})
            cd.add(f"{name}/{label}", "sched", ints, arrays)
    # calls that are answered before anything is touched
    random.seed(5)
    random.getrandbits(32)
    words, index = _py_state()
    ok = dict(n_train=20, n_pool=6, batch_size=4, n_pseudo=3, batches_per_epoch=5, in_epoch=5, index=index, count=2, alloc_count=2, expect_rc=-1)
    good_pool = [5, 9, 11, 200, 7, 8]
    for label, ints, pool in (
            ("pool_shorter_than_n_pseudo", dict(n_pseudo=7), good_pool),
            ("pool_id_above_int32", {}, [5, 9, 11, INT32_MAX + 1, 7, 8]),
            ("negative_pool_id", {}, [5, 9, 11, 200, 7, -1]),
            ("null_generator", dict(null_arg=1), good_pool), ("null_train", dict(null_arg=2), good_pool),
            ("null_pool", dict(null_arg=3), good_pool), ("null_in_epoch", dict(null_arg=4), good_pool),
            ("null_out_nodes", dict(null_arg=5), good_pool), ("null_out_len", dict(null_arg=6), good_pool),
            ("count_0", dict(count=0, expect_rc=0), good_pool), ("count_negative", dict(count=-1), good_pool),
            ("batch_size_0", dict(batch_size=0), good_pool), ("batches_per_epoch_0", dict(batches_per_epoch=0), good_pool)):
        cd.add("refused/" + label, "sched_refused", dict(ok, **ints),
               dict(train=(list(range(20)), np.int64), pool=(pool, np.int64), state=(words, np.uint32)))
    return cd.close()


# ---- the per-shuffle entry points, the set order, the neighbour sampler ----------------------------------------------------------------

SHUFFLE_N = (0, 1, 2, 3, 63, 64, 65, 623, 624, 625, 4097, 55275)
SEEDS = (0, 1, 72, 2 ** 32, 2 ** 63 + 11)


def _setsize(k):
    return 21 if k <= 5 else 21 + 4 ** math.ceil(math.log(k * 3, 4))          # Lib/random.py, sample()


def _graph(degrees, rng):
    """CSR whose row r has degrees[r] distinct ascending columns spread over [0, n); rows behind the list are empty."""
    n = max(len(degrees) + 3, max(degrees) * 3 + 5)
    rowptr = np.zeros(n + 1, dtype=np.int32)
    cols = []
    for r in range(n):
        d = degrees[r] if r < len(degrees) else 0
        cols.append(np.sort(rng.choice(n, size=d, replace=False)).astype(np.int32))
        rowptr[r + 1] = rowptr[r] + d
    return rowptr, np.concatenate(cols)


def _adj(rowptr, col):
    """the sets the reference samples from, filled in ascending order (ggad_amd/synth.py::csr_to_adj_lists)."""
    return [set(int(c) for c in col[rowptr[v]:rowptr[v + 1]]) for v in range(len(rowptr) - 1)]


def _sample_table(adj, nodes, k):
    """`random.sample(tuple(adj[v]), k)` per row, sorted, padded with -1; a row shorter than k is taken whole and draws nothing."""
    nbr = np.full((len(nodes), k), -1, dtype=np.int32)
    cnt = np.zeros(len(nodes), dtype=np.int32)
    for r, v in enumerate(nodes):
        s = adj[v]
        row = sorted(random.sample(tuple(s), k)) if len(s) >= k else sorted(s)
        nbr[r, :len(row)] = row
        cnt[r] = len(row)
    return nbr, cnt


def _entry_point_cases(path):
    cd = CaseDir(path)
    # random.seed + two shuffles of one list (the second starts mid-block), in one call each and as targets + swaps
    for seed in SEEDS:
        for n in SHUFFLE_N:
            random.seed(seed)
            seeded_w, seeded_i = _py_state()
            lst = [10 * i - 77 for i in range(n)]
            want = list(lst)
            random.shuffle(want)
            random.shuffle(want)
            w, ix = _py_state()
            for mode in (0, 1):
                cd.add(f"shuffle/seed{seed}/n{n}/mode{mode}", "shuffle",
                       dict(seed_lo=seed & 0xffffffff, seed_hi=seed >> 32, n=n, reps=2, mode=mode, index_seeded=seeded_i, index_out=ix),
                       dict(data=(lst, np.int64), data_out=(want, np.int64), state_seeded=(seeded_w, np.uint32), state_out=(w, np.uint32)))
    # set_state / get_state, and the raw outputs across two block boundaries
    for seed, skip, draws in ((72, 0, 1300), (2 ** 63 + 11, 600, 30)):
        random.seed(seed)
        for _ in range(skip):
            random.getrandbits(32)
        w0, i0 = _py_state()
        bits = [random.getrandbits(32) for _ in range(draws)]
        w1, i1 = _py_state()
        cd.add(f"state/seed{seed}", "state", dict(index=i0, draws=draws, index_out=i1),
               dict(state=(w0, np.uint32), bits=(bits, np.uint32), state_out=(w1, np.uint32)))
    # the iteration order of a set filled in ascending order: the first resizes (5 and 9 keys.. ), the 50,000 growth rule, gaps, both ends
    for n in (0, 1, 4, 5, 8, 9, 10000, 60000):
        for label, keys in (("dense", np.arange(n, dtype=np.int64)),
                            ("gaps", np.arange(n, dtype=np.int64) * 32768 + 7),
                            ("ends", np.concatenate(([0], INT32_MAX - np.arange(n - 1, dtype=np.int64)[::-1] * 1021)) if n else np.zeros(0, dtype=np.int64))):
            assert len(keys) == n and (n == 0 or (keys.min() >= 0 and keys.max() <= INT32_MAX)) and (np.diff(keys) > 0).all()
            s = set()
            for c in keys.tolist():
                s.add(c)
            cd.add(f"pyset/{label}/n{n}", "pyset", dict(n=n, expect_rc=0), dict(keys=(keys, np.int32), order=(list(s), np.int32)))
    for label, keys in (("unsorted", [1, 5, 4, 9]), ("duplicate", [1, 5, 5, 9]), ("negative", [-1, 2, 3]), ("negative_later", [0, 2, -3])):
        cd.add(f"pyset/refused/{label}", "pyset", dict(n=len(keys), expect_rc=-1), dict(keys=(keys, np.int32)))
    # ggad_mt_sample_rows
    for k in (1, 5, 6, 25):
        ss = _setsize(k)
        degrees = sorted(set(d for d in (k - 1, k, k + 1, 20, 21, 22, ss - 1, ss, ss + 1, 300, 0) if d >= 0))
        rowptr, col = _graph(degrees, np.random.default_rng(k))
        adj = _adj(rowptr, col)
        n_nodes = len(rowptr) - 1
        nodes = list(range(len(degrees))) + [len(degrees) - 1, 0, len(degrees) - 1, n_nodes - 1] + list(range(len(degrees)))[::-1]
        random.seed(1000 + k)
        random.getrandbits(32)
        w0, i0 = _py_state()
        nbr, cnt = _sample_table(adj, nodes, k)
        w1, i1 = _py_state()
        ints = dict(n_nodes=n_nodes, n_rows=len(nodes), nnz=len(col), k=k, setsize=ss, index=i0, index_out=i1, expect_rc=0)
        arrs = dict(rowptr=(rowptr, np.int32), col=(col, np.int32), nodes=(nodes, np.int64), state=(w0, np.uint32), state_out=(w1, np.uint32),
                    nbr=(nbr, np.int32), cnt=(cnt, np.int32))
        cd.add(f"sample_rows/k{k}", "sample_rows", ints, arrs)
        refused = dict(ints, expect_rc=-1)
        bad_col = col.copy()
        a = int(rowptr[len(degrees) - 1])                                   # the longest row
        bad_col[a], bad_col[a + 1] = bad_col[a + 1], bad_col[a]
        neg_col = col.copy()
        neg_col[a] = -1
        last_bad = nodes[:-1] + [n_nodes]
        for label, ri, ra in (("id_outside", {}, dict(nodes=(last_bad, np.int64))),
                              ("negative_id", {}, dict(nodes=([-1] + nodes[1:], np.int64))),
                              ("unsorted_row", {}, dict(col=(bad_col, np.int32))),
                              ("negative_column", {}, dict(col=(neg_col, np.int32))),
                              ("k_0", dict(k=0, k_alloc=k), {}), ("setsize_20", dict(setsize=20), {}), ("n_nodes_0", dict(n_nodes_arg=0), {}),
                              ("null_generator", dict(null_arg=1), {}), ("null_rowptr", dict(null_arg=2), {}), ("null_nodes", dict(null_arg=3), {}),
                              ("null_nbr", dict(null_arg=4), {}), ("null_cnt", dict(null_arg=5), {})):
            cd.add(f"sample_rows/k{k}/refused/{label}", "sample_rows", dict(refused, **ri), dict(arrs, **ra))
    # ggad_sage_sched_epoch
    for k, n_train, n_pool, bs, n_pseudo, nb, extra, checked in (
            (1, 37, 9, 8, 3, 5, 0, 0),           # ragged last batch (37 = 4 * 8 + 5)
            (5, 24, 2, 8, 4, 4, 7, 1),           # a pool shorter than n_pseudo is taken whole; the last batch starts behind train; gaps in the table
            (6, 20, 12, 6, 5, 3, 0, 0),          # (only the first 18 of the shuffled train ids are used)
            (25, 10, 30, 16, 6, 1, 3, 1),        # n_train < batch_size
            (5, 0, 6, 4, 3, 2, 0, 0),            # no train ids at all
            (5, 9, 0, 4, 3, 3, 0, 0)):           # no pool (9 = 2 * 4 + 1)
        ss = _setsize(k)
        degrees = [d for d in (k - 1, k, k + 1, 21, 22, ss, ss + 1, 0, 60) if d >= 0] * 5
        rowptr, col = _graph(degrees, np.random.default_rng(100 + k))
        adj = _adj(rowptr, col)
        n_nodes = len(rowptr) - 1
        rng = np.random.default_rng(7 * k)
        labels = rng.integers(0, 2, n_nodes)
        ids = rng.permutation(len(degrees))
        train = ids[:n_train].tolist()
        pool = (ids[n_train:n_train + n_pool].tolist() + [train[0] if train else 0] * n_pool)[:n_pool]      # (a node may be in both lists)
        pool[-1:] = pool[:1] if n_pool > 1 else pool[-1:]                    # ... and twice in one
        b_max = bs + n_pseudo
        stride = b_max * (3 + k) + extra
        table_len = (nb - 1) * stride + b_max * (3 + k)
        random.seed(50 + k + n_train)
        for _ in range(3 * k):
            random.getrandbits(32)
        w0, i0 = _py_state()
        tr, po = list(train), list(pool)
        table = np.full(table_len, CANARY32, dtype=np.int32)
        lens = []
        random.shuffle(tr)
        for b in range(nb):
            random.shuffle(po)
            nodes = tr[b * bs:min(b * bs + bs, n_train)] + po[:n_pseudo]
            nbr, cnt = _sample_table(adj, nodes, k)
            t = table[b * stride:b * stride + b_max * (3 + k)]
            t[:] = 0
            t[3 * b_max:] = -1
            t[:len(nodes)] = nodes
            t[b_max:b_max + len(nodes)] = cnt
            t[2 * b_max:2 * b_max + len(nodes)] = labels[nodes] if nodes else []
            t[3 * b_max:3 * b_max + len(nodes) * k] = nbr.reshape(-1)
            lens.append(len(nodes))
        w1, i1 = _py_state()
        ints = dict(n_train=n_train, n_pool=n_pool, batch_size=bs, n_pseudo=n_pseudo, num_batches=nb, n_nodes=n_nodes, nnz=len(col), k=k, setsize=ss,
                    checked=checked, stride=stride, table_len=table_len, len_alloc=nb, index=i0, index_out=i1, expect_rc=0)
        arrs = dict(train=(train, np.int64), pool=(pool, np.int64), rowptr=(rowptr, np.int32), col=(col, np.int32), labels=(labels, np.int64),
                    state=(w0, np.uint32), state_out=(w1, np.uint32), table=(table, np.int32), len_out=(lens, np.int32),
                    train_out=(tr, np.int64), pool_out=(po, np.int64))
        name = f"sage_epoch/k{k}_t{n_train}_p{n_pool}_c{checked}"
        cd.add(name, "sage_epoch", ints, arrs)
        if n_train == 0 or n_pool == 0:
            continue
        refused = dict(ints, expect_rc=-1, checked=0)
        bad_col = col.copy()
        v = max(train, key=lambda u: len(adj[u]))                           # a train id with a row of two entries at least
        a = int(rowptr[v])
        bad_col[a], bad_col[a + 1] = bad_col[a + 1], bad_col[a]
        for label, ri, ra in (("train_id_outside", {}, dict(train=(train[:-1] + [n_nodes], np.int64))),
                              ("pool_id_negative", {}, dict(pool=([-1] + pool[1:], np.int64))),
                              ("unsorted_row_of_a_train_id", {}, dict(col=(bad_col, np.int32))),
                              ("k_0", dict(k=0), {}), ("stride_short", dict(stride=b_max * (3 + k) - 1), {}),
                              ("num_batches_0", dict(num_batches=0), {}), ("batch_size_0", dict(batch_size=0), {}),
                              ("null_generator", dict(null_arg=1), {}), ("null_rowptr", dict(null_arg=2), {}), ("null_labels", dict(null_arg=3), {}),
                              ("null_table", dict(null_arg=4), {}), ("null_len", dict(null_arg=5), {})):
            cd.add(f"{name}/refused/{label}", "sage_epoch", dict(refused, **ri), dict(arrs, **ra))
    # a batch of zero rows: no pool, and the last batch starts behind the end of train
    # (9 train ids in batches of 4: batch 3 of 4 would be train[12:16]); everything else about the call is valid
    k, bs, n_pseudo, nb = 5, 4, 3, 4
    rowptr, col = _graph([7, 3, 0, 12, 5, 6, 30, 4, 9, 22], np.random.default_rng(9))
    n_nodes, b_max = len(rowptr) - 1, bs + n_pseudo
    random.seed(9)
    w0, i0 = _py_state()
    cd.add("sage_epoch/refused/batch_of_zero_rows", "sage_epoch",
           dict(n_train=9, n_pool=0, batch_size=bs, n_pseudo=n_pseudo, num_batches=nb, n_nodes=n_nodes, nnz=len(col), k=k, setsize=_setsize(k), checked=0,
                stride=b_max * (3 + k), table_len=nb * b_max * (3 + k), len_alloc=nb, index=i0, expect_rc=-1),
           dict(train=(list(range(9)), np.int64), pool=([], np.int64), rowptr=(rowptr, np.int32), col=(col, np.int32),
                labels=(np.zeros(n_nodes, dtype=np.int64), np.int64), state=(w0, np.uint32)))
    return cd.close()


# ---- the plan builders: record at the C boundary, replay -----------------------------------------------------------------------------

def _host_array(ptr, n, dtype):
    nbytes = int(n) * np.dtype(dtype).itemsize
    if nbytes == 0:
        return np.zeros(0, dtype=dtype)
    return np.frombuffer((ctypes.c_char * nbytes).from_address(int(ptr)), dtype=dtype).copy()


class RecordingLib:
    """What `_lib.load()` returns, with the five host builder entry points recording their arguments and outputs."""

    def __init__(self, lib):
        self._lib = lib
        self.shape = None          # of the matrix whose plan is being built: rowptr holds shape[0] + 1 offsets
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        rec = getattr(self, "_rec_" + name, None) if name.startswith("ggad_spmm_") else None
        if rec is None:
            return fn

        def call(*args):
            rc = fn(*args)
            self.calls.append(rec(rc, *args))
            return rc
        return call

    def _common(self, rowptr, col, n_rounds, round_rows, round_wide, skip_diag, n_threads):
        n_rows = self.shape[0]
        rp = _host_array(rowptr, n_rows + 1, np.int64)
        ints = dict(n_rows=n_rows, nnz=int(rp[-1]), n_rounds=n_rounds, skip_diag=skip_diag, n_threads=n_threads)
        arrs = dict(rowptr=(rp, np.int64), col=(_host_array(col, rp[-1], np.int32), np.int32), round_rows=(_host_array(round_rows, n_rounds * 8, np.int32), np.int32))
        if round_wide:
            arrs["round_wide"] = (_host_array(round_wide, n_rounds, np.int32), np.int32)
        return ints, arrs

    def _rec_ggad_spmm_panel_count(self, rc, rowptr, col, n_rounds, round_rows, round_wide, skip_diag, R, NC, steps_rc, n_threads):
        ints, arrs = self._common(rowptr, col, n_rounds, round_rows, round_wide, skip_diag, n_threads)
        ints.update(panel_rows=R, n_panels=NC, n_out=n_rounds * NC, expect_rc=rc)
        arrs["steps_rc"] = (_host_array(steps_rc, n_rounds * NC, np.int32), np.int32)
        return "panel_count", ints, arrs

    def _rec_ggad_spmm_panel_fill(self, rc, rowptr, col, n_rounds, round_rows, round_wide, skip_diag, R, NC, steps_rc, tile_oct, stream, total, spare, n_threads):
        ints, arrs = self._common(rowptr, col, n_rounds, round_rows, round_wide, skip_diag, n_threads)
        ints.update(panel_rows=R, n_panels=NC, total_octs=total, spare_octs=spare, expect_rc=rc)
        arrs.update(steps_rc=(_host_array(steps_rc, n_rounds * NC, np.int32), np.int32), tile_oct=(_host_array(tile_oct, n_rounds * NC, np.int64), np.int64),
                    stream=(_host_array(stream, (total + spare) * 64, np.uint16), np.uint16))
        return "panel_fill", ints, arrs

    def _rec_ggad_spmm_panel_values_factor(self, rc, rowptr, col, val, r, n, rtol, n_threads):
        rp = _host_array(rowptr, n + 1, np.int64)
        return "values_factor", dict(n_rows=n, nnz=int(rp[-1]), n_threads=n_threads, expect_rc=rc), dict(
            rowptr=(rp, np.int64), col=(_host_array(col, rp[-1], np.int32), np.int32), val=(_host_array(val, rp[-1], np.float32), np.float32),
            r=(_host_array(r, n, np.float64), np.float64), rtol=([rtol], np.float64))

    def _rec_ggad_spmm_ring_count(self, rc, rowptr, col, n_rounds, round_rows, round_wide, skip_diag, RS, S, V, NP, quads, n_threads):
        ints, arrs = self._common(rowptr, col, n_rounds, round_rows, round_wide, skip_diag, n_threads)
        ints.update(slot_rows=RS, n_ring_slots=S, window=V, n_phases=NP, n_out=n_rounds * NP, expect_rc=rc)
        arrs["quads_rp"] = (_host_array(quads, n_rounds * NP, np.uint16), np.uint16)
        return "ring_count", ints, arrs

    def _rec_ggad_spmm_ring_fill(self, rc, rowptr, col, n_rounds, round_rows, round_wide, skip_diag, RS, S, V, NP, quads, quad_off, idx, n_sb, n_threads):
        ints, arrs = self._common(rowptr, col, n_rounds, round_rows, round_wide, skip_diag, n_threads)
        ints.update(slot_rows=RS, n_ring_slots=S, window=V, n_phases=NP, n_sb=n_sb, n_tiles=n_rounds * NP, expect_rc=rc)
        arrs.update(quads_rp=(_host_array(quads, n_rounds * NP, np.uint16), np.uint16), quad_off=(_host_array(quad_off, n_rounds * NP, np.int64), np.int64),
                    idx=(_host_array(idx, n_sb * 128, np.uint16), np.uint16))
        return "ring_fill", ints, arrs


def _builder_cases(path, monkeypatch):
    real = _lib.load()
    rec = RecordingLib(real)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    marks = {}

    def plans(label, m, n_slices, rows=None, panel=True, ring=True):
        first = len(rec.calls)
        rec.shape = m.shape
        csr = Csr(m, "cpu")
        if panel:
            assert csr.panel_plan(n_slices, rows, None if rows is None else {}) is not None, label
        if ring:
            assert csr.ring_plan(n_slices, rows, None if rows is None else {}) is not None, label
        marks[label] = (first, len(rec.calls))

    R, RS = int(real.ggad_spmm_panel_rows()), int(real.ggad_spmm_ring_slot_rows())
    # the matrices of tests/test_fullgraph_{panel,ring}_cpu.py: normalised adjacency + I, the diagonal kept out of the stream (hub rows
    # become WIDE rounds; more than 256 rounds: the builders split them over four threads) ...
    n = 2 * R + 452
    big = _normalized(n, 0.05, 3, False)
    plans("normalized", big, 3)
    plans("normalized_loops_inside", _normalized(RS + 301, 0.05, 4, True), 2)
    # ... and a 0/1 pattern matrix with its diagonal in the stream; a row subset that repeats a row and ends in a round padded with -1
    pat = (_normalized(1500, 0.08, 5, False) != 0).astype(np.float64).tocsr()
    plans("pattern", pat, 2)
    plans("pattern_row_subset", pat, 2, np.array([7, 1499, 3, 3, 640, 0] + list(range(100, 160))))
    # rectangular, shorter than one panel / one ring slot, with an empty row and a last round padded with -1
    small = sp.random(123, 90, density=0.5, random_state=np.random.default_rng(4), format="lil")
    small[17, :] = 0
    small = small.tocsr()
    small.eliminate_zeros()
    small.data[:] = 1.0
    assert small.shape[1] < min(R, RS) and small.indptr[17] == small.indptr[18]
    plans("small_rectangular", small, 1)
    monkeypatch.undo()

    cd = CaseDir(path)
    seen_ops = set()
    for label, (a, b) in marks.items():
        for i, (op, ints, arrs) in enumerate(rec.calls[a:b]):
            assert ints["expect_rc"] >= 0
            seen_ops.add(op)
            cd.add(f"{label}/{i}_{op}", op, ints, arrs)
            if label == "normalized" and op != "values_factor":             # the thread split: byte-equal for one thread and for four
                assert ints["n_rounds"] >= 256
                for nt in (1, 4):
                    cd.add(f"{label}/{i}_{op}/threads{nt}", op, dict(ints, n_threads=nt), arrs)
            if label == "normalized" and op == "values_factor":
                for nt in (1, 4):
                    cd.add(f"{label}/{i}_{op}/threads{nt}", op, dict(ints, n_threads=nt), arrs)
    assert seen_ops == {"panel_count", "panel_fill", "values_factor", "ring_count", "ring_fill"}
    wide = [c for c in rec.calls[slice(*marks["normalized"])] if c[0] == "panel_fill"][0][2]["round_wide"][0]
    assert wide.sum() >= 8, "the hub rows did not become WIDE rounds"
    # values that do not factor: the verdict 0
    w = big.copy()
    w.data = w.data * np.random.default_rng(2).uniform(0.5, 1.5, size=w.nnz)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    first = len(rec.calls)
    rec.shape = w.shape
    assert Csr(w, "cpu").value_factors() is False
    monkeypatch.undo()
    for i, (op, ints, arrs) in enumerate(rec.calls[first:]):
        assert op == "values_factor" and ints["expect_rc"] == 0
        cd.add(f"unfactorable/{i}_{op}", op, ints, arrs)
    # invalid arguments: refused before anything is written
    for label in ("small_rectangular", "pattern_row_subset"):
        padded = [c[2]["round_rows"][0] for c in rec.calls[slice(*marks[label])] if c[0] in ("panel_fill", "ring_fill")]
        assert len(padded) >= 2 and all((rr.reshape(-1, 8)[-1] == -1).any() and (rr.reshape(-1, 8)[-1] >= 0).any() for rr in padded), \
            f"{label}: no round padded with -1 rows"
    # (the all-ones small matrix never asks whether its values factor: that call comes from a normalised one)
    base = rec.calls[slice(*marks["small_rectangular"])] + [c for c in rec.calls[slice(*marks["normalized_loops_inside"])] if c[0] == "values_factor"][:1]
    refused_ops = {}
    for op, ints, arrs in base:
        bad = {"panel_count": [dict(null_arg=1), dict(null_arg=2), dict(null_arg=3), dict(null_arg=4), dict(n_rounds_arg=-1), dict(panel_rows=0), dict(n_panels=0)],
               "panel_fill": [dict(null_arg=k) for k in range(1, 7)] + [dict(panel_rows=1), dict(panel_rows=65001)],
               "values_factor": [dict(null_arg=k) for k in range(1, 5)] + [dict(n_rows_arg=-1)],
               "ring_count": [dict(null_arg=k) for k in range(1, 5)] + [dict(n_rounds_arg=-1), dict(slot_rows=1), dict(n_ring_slots=1), dict(window=0),
                                                                         dict(window=ints.get("n_ring_slots", 0)), dict(n_phases=0)],
               "ring_fill": [dict(null_arg=k) for k in range(1, 7)] + [dict(slot_rows=ints.get("slot_rows", 0) + 1), dict(n_ring_slots=1), dict(window=0),
                                                                        dict(window=ints.get("n_ring_slots", 0)), dict(slot_rows=32768, n_ring_slots=2)]}[op]
        for change in bad:
            tag = "_".join(f"{k}{v}" for k, v in change.items())
            cd.add(f"invalid/{op}/{tag}", op, dict(ints, expect_rc=-1, **change), arrs)
            refused_ops[op] = refused_ops.get(op, 0) + 1
    assert set(refused_ops) == seen_ops and min(refused_ops.values()) >= 5, refused_ops      # every entry point has its refusals
    return cd.close()


# ---- the tests ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sched_cases(tmp_path_factory):
    return _sched_cases(tmp_path_factory.mktemp("sched"))


@pytest.fixture(scope="module")
def entry_point_cases(tmp_path_factory):
    return _entry_point_cases(tmp_path_factory.mktemp("entry_points"))


@pytest.fixture(scope="module")
def builder_cases(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    try:
        return _builder_cases(tmp_path_factory.mktemp("builders"), mp)
    finally:
        mp.undo()


@pytest.mark.parametrize("link", ["avx2", "scalar"])
def test_sampler_entry_points(toolchain, link, entry_point_cases):
    """ggad_mt_seed_u64 / set_state / get_state / getrandbits32, ggad_mt_shuffle_i64, ggad_mt_shuffle_targets + ggad_apply_swaps_i64,
    ggad_pyset_order_i32, ggad_mt_sample_rows and ggad_sage_sched_epoch against the running interpreter, every refusal with canaries in the
    outputs; with the AVX2 kernels and with the scalar fall-backs (the expected bytes are the same files: both links give the same)."""
    case_dir, n = entry_point_cases
    toolchain.run(toolchain.sampler(link), case_dir, n)


@pytest.mark.parametrize("switches", list(SWITCHES))
@pytest.mark.parametrize("link", ["avx2", "scalar"])
def test_sched_batches_pipeline(toolchain, link, switches, sched_cases):
    """ggad_sched_batches against the per-batch loop of the header on `random`: every configuration of SCHED_CONFIGS in one call and cut
    into three, final lists / epoch counter / generator state after every call, and the calls it must answer without touching anything.
    One process per setting of GGAD_SCHED_C / GGAD_SCHED_M / GGAD_SCHED_PIN (read once per process); the outputs do not depend on them."""
    case_dir, n = sched_cases
    toolchain.run(toolchain.sampler(link), case_dir, n, SWITCHES[switches])


def test_plan_builders(toolchain, builder_cases):
    """ggad_spmm_panel_count / _fill / _values_factor and ggad_spmm_ring_count / _fill replayed on exact allocations: outputs equal the
    production library's byte for byte, for the recorded thread count and for 1 and 4 threads; the read-ahead region behind the last tile
    names zero rows only; invalid arguments leave the outputs untouched."""
    case_dir, n = builder_cases
    toolchain.run(toolchain.builder(), case_dir, n)
