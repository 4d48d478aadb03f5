"""No GPU: the arithmetic of the device-resident L-BFGS minimiser (torchmd-net_amd/csrc/tn_lbfgs_math.h, compiled for the host by
tests/lbfgs_host.hip) against tests/lbfgs_oracle.py.  1. the coefficient-space recursion against the two loops on the vectors, on a
table of scripted histories and on the wells, within 64 x the error recorded in profiles/minimize_lbfgs.json; 2. the integer state
(pairs held, ring order, accepted, converged_at) and the clamp; 3. the wells in both precisions; 4. the non-convex well: the same pairs
rejected; 5. the sanitizers on a stand-alone program; 6. signatures and exports.

``python -m tests.test_lbfgs_host`` measures 1. and writes it to profiles/minimize_lbfgs.json (``gram_vs_two_loop``)."""
import inspect
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import lbfgs_host_mirror as H
from tests import lbfgs_oracle as O
from tests import min_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "minimize_lbfgs.json")
P = dict(O.LBFGS, fmax=1e-3)
FIXED = [2, 50, 51, 700, 1607]


def _problem():
    batch, kspring, x0, x = MO.wells_problem(interleave=True)
    fixed = np.zeros(len(batch), np.uint8)
    fixed[FIXED] = 1
    return batch, kspring, x0, x, fixed


def _p64(st, m, f):
    """p of molecule m from the header's coefficients, in fp64 and unrounded: -(delta_g g + sum (delta_s s + delta_y y))"""
    mine = st.batch == m
    free = np.ones(mine.sum(), bool) if st.fixed is None else st.fixed[mine] == 0
    g = -np.where(free[:, None], np.asarray(f, np.float64)[mine], 0.0).ravel()
    acc = st.delta[m, 2 * st.M1] * g
    for a in st.order[m, :st.h[m]]:
        acc = acc + st.delta[m, a] * st.S[a][mine].astype(np.float64).ravel()
        acc = acc + st.delta[m, st.M1 + a] * st.Y[a][mine].astype(np.float64).ravel()
    return -acc, g


def _recursion_error(st, f):
    """max over the moving molecules of max |p_header - p_two_loop| / max |p|, the two loops on the header's own stored pairs"""
    worst = 0.0
    for m in range(st.n_mol):
        if st.conv[m] >= 0 or not (st.batch == m).any():
            continue
        p, g = _p64(st, m, f)
        S, Y = st.pairs(m)
        ref = O.two_loop(S, Y, g, st.p["alpha"])
        if np.abs(ref).max() > 0:
            worst = max(worst, float(np.abs(p - ref).max() / np.abs(ref).max()))
    return worst


class _Both:
    """The header's state and one oracle molecule per molecule, stepped together on forces the caller supplies.  The oracle takes the
    header's stored candidate (fp32, widened), so its decisions are made on the same numbers."""

    def __init__(self, batch, n_mol, p, x, fixed=None):
        self.st = H.State(batch, n_mol, p, fixed)
        free = np.ones(len(batch), bool) if fixed is None else np.asarray(fixed) == 0
        self.idx = [np.nonzero(np.asarray(batch) == m)[0] for m in range(n_mol)]
        self.mols = [O.Molecule(p, free[self.idx[m]]) for m in range(n_mol)]
        self.x, self.f, self.step, self.err = np.asarray(x, np.float32).copy(), None, 0, 0.0

    def control(self, f):
        """the launches after an evaluation: sums, control, direction; then the comparisons -> ret"""
        st = self.st
        self.f = np.asarray(f, np.float32)
        fresh = st.fresh
        before = [(st.h[m], st.order[m].copy()) for m in range(st.n_mol)]
        st.sums(self.x, self.f)
        ret = st.control(self.step).copy()
        if (ret == O.UNUSABLE).any():
            return ret
        st.direct(self.f)
        for m, mol in enumerate(self.mols):
            i = self.idx[m]
            was_frozen = mol.converged_at >= 0
            spare = before[m][1][before[m][0]]
            r, p_ref, c_ref = mol.control(self.x[i], self.f[i], self.step,
                                          pair=None if fresh or was_frozen else (st.S[spare][i], st.Y[spare][i]))
            assert r == ret[m], (self.step, m, r, ret[m])
            assert mol.converged_at == st.conv[m] and mol.accepted == st.accepted[m], (self.step, m)
            if was_frozen:
                continue
            assert mol.h == st.h[m], (self.step, m, mol.h, st.h[m])
            assert sorted(st.order[m]) == list(range(st.M1))  # the ring order stays a permutation of the slots
            S, Y = st.pairs(m)
            for k in range(mol.h):  # the same pairs, oldest first
                assert np.array_equal(S[k], mol.s[k].ravel()) and np.array_equal(Y[k], mol.y[k].ravel()), (self.step, m, k)
        self.err = max(self.err, _recursion_error(st, self.f))
        return ret

    def move(self):
        """the move: x <- x + c p with the header's c; the clamp within 1 fp32 ulp of the oracle's on the header's own direction"""
        st = self.st
        self.x = st.move(self.x, self.f)
        for m, mol in enumerate(self.mols):
            i = self.idx[m]
            mol.moved(st.x_prev[i], st.f_prev[i])
            if st.conv[m] < 0 and len(i):
                c_ref = np.float32(O.clamp(st.direction[i].astype(np.float64), st.p))
                assert MO.ulp_distance(st.scale[m], c_ref) <= 1, (self.step, m, st.scale[m], c_ref)
            else:
                assert st.scale[m] == 0
        self.step += 1


def _scripted(memory, script, seed=0, fmax=1e-6):
    """Two interleaved molecules of 5 and 9 atoms, one atom fixed, driven by a script: per step and molecule 'a' (the next pair has
    y = K s, K > 0: accepted) or 'r' (y = -K s: rejected).  -> the _Both after the last control"""
    rng = np.random.default_rng(seed)
    batch = np.array([0, 1, 1, 0, 1, 1, 0, 1, 0, 1, 1, 0, 1, 1])
    fixed = np.zeros(len(batch), np.uint8)
    fixed[4] = 1
    p = dict(O.LBFGS, memory=memory, fmax=fmax)
    x = rng.normal(size=(len(batch), 3)).astype(np.float32)
    K = rng.uniform(0.5, 20.0, size=(len(batch), 3))
    both = _Both(batch, 2, p, x, fixed)
    f = rng.normal(size=x.shape).astype(np.float32)
    both.control(f)
    for row in script:
        both.move()
        sign = np.array([1.0 if row[m] == "a" else -1.0 for m in batch])[:, None]
        s = both.x.astype(np.float64) - both.st.x_prev
        f = (both.st.f_prev - sign * K * s).astype(np.float32)
        both.control(f)
        for m in range(2):
            assert both.st.accepted[m] == (row[m] == "a"), (row, m)
    return both


TABLE = {
    "h0_h1": (3, ["aa"]),
    "fill_memory_3": (3, ["aa", "aa", "aa"]),
    "wrap_memory_1": (1, ["aa"] * 9),
    "wrap_memory_3": (3, ["aa"] * 10),
    "reject_below_memory": (3, ["aa", "rr", "aa", "ra", "ar"]),
    "reject_at_memory": (3, ["aa", "aa", "aa", "rr", "aa", "ra", "ar", "aa"]),
    "reject_at_memory_1": (1, ["aa", "rr", "ar", "ra", "aa"]),
    "memory_100_never_full": (100, ["aa"] * 12),
}


def _wells_run(p, anharmonic, max_steps, record=None):
    """the wells through the header step by step (fp32), the forces from tests/lbfgs_oracle.py in fp32 -> the _Both, steps taken"""
    batch, kspring, x0, x, fixed = _problem()
    both = _Both(batch, 5, p, x, fixed)
    k32, x032 = kspring.astype(np.float32), x0.astype(np.float32)
    while True:
        f = O.well_forces(k32, x032, both.x, np.float32(anharmonic)).astype(np.float32)
        both.control(f)
        if record is not None:
            record.append((both.st.h.copy(), both.st.accepted.copy(), both.st.conv.copy()))
        if (both.st.conv >= 0).all() or both.step == max_steps:
            return both, both.step
        both.move()


def measure():
    """max |p_header - p_two_loop| / max |p| per case -> dict"""
    out = {}
    for name, (memory, script) in TABLE.items():
        out[name] = _scripted(memory, script).err
    for memory in (1, 3, 100):
        out[f"wells_memory_{memory}"] = _wells_run(dict(P, memory=memory), 0.0, 200)[0].err
        out[f"wells_anharmonic_2_memory_{memory}"] = _wells_run(dict(P, memory=memory), 2.0, 400)[0].err
    return out


def _recorded():
    with open(PROFILE) as fh:
        return json.load(fh)["gram_vs_two_loop"]


# ---- 1. / 2. the recursion, the integer state, the clamp --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TABLE))
def test_recursion_and_state_on_the_table(name):
    """every step: pairs held, ring order, accepted flag, converged_at and the stored pairs equal the oracle's (in _Both.control); the
    clamp within 1 fp32 ulp (in _Both.move); the coefficient-space direction within 64 x the recorded error of the two loops.  The
    bound: the error was measured on this table and the wells on the CPU; the device's summation order differs and the conditioning
    varies from case to case, hence the factor 64.  A recorded value that is not far below 2^-24 would mean the formulation is wrong."""
    rec = _recorded()
    assert rec["max"] < 2.0 ** -24 / 1024
    memory, script = TABLE[name]
    both = _scripted(memory, script)
    print(name, "measured", both.err, "bound", 64 * rec["max"])
    assert both.err <= 64 * rec["max"]
    assert both.step == len(script)


def test_rejected_candidate_at_full_memory_keeps_the_oldest_pair():
    """memory 3, three pairs held, then a rejected candidate: the three pairs, the oldest included, are what they were, bit for bit"""
    a = _scripted(3, ["aa", "aa", "aa"])
    b = _scripted(3, ["aa", "aa", "aa", "rr"])
    for m in range(2):
        assert a.st.h[m] == b.st.h[m] == 3 and np.array_equal(a.st.order[m], b.st.order[m])
        for u, v in zip(a.st.pairs(m)[0] + a.st.pairs(m)[1], b.st.pairs(m)[0] + b.st.pairs(m)[1]):
            assert np.array_equal(u, v)
        assert np.array_equal(a.st.SS[m], b.st.SS[m]) and np.array_equal(a.st.SY[m], b.st.SY[m]) and np.array_equal(a.st.YY[m], b.st.YY[m])
    c = _scripted(3, ["aa", "aa", "aa", "aa"])  # an accepted one instead: the oldest pair has left
    assert not np.array_equal(c.st.pairs(0)[0][0], a.st.pairs(0)[0][0]) and np.array_equal(c.st.pairs(0)[0][0], a.st.pairs(0)[0][1])


def test_first_direction_is_the_scaled_force():
    """h = 0: p = F / alpha (0 for the fixed atom), and g.p = -ff / alpha"""
    both = _scripted(3, [])
    st = both.st
    want = (both.f.astype(np.float64) / 70.0).astype(np.float32)
    want[4] = 0
    assert np.array_equal(st.direction, want) and (st.h == 0).all()
    for m in range(2):
        assert abs(st.gp[m] + st.tot[m, 6 * st.M1] / 70.0) <= 2.0 ** -52 * st.tot[m, 6 * st.M1]


def test_a_converged_molecule_is_frozen():
    """fmax above every force: both molecules converge at step 0, no pair is ever held, x keeps its bits; a NaN force is then not
    looked at"""
    rng = np.random.default_rng(1)
    batch = np.array([0, 1, 1, 0, 1])
    x = rng.normal(size=(5, 3)).astype(np.float32)
    both = _Both(batch, 2, dict(O.LBFGS, memory=3, fmax=1e6), x)
    f = rng.normal(size=x.shape).astype(np.float32)
    assert (both.control(f) == O.FROZEN).all() and (both.st.conv == 0).all()
    both.move()
    assert np.array_equal(both.x, x) and (both.st.scale == 0).all()
    f[1, 1] = np.nan
    assert (both.control(f) == O.FROZEN).all() and (both.st.conv == 0).all() and (both.st.h == 0).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_sum_that_is_not_finite_is_unusable(bad):
    """nothing of that molecule is written: pairs held, ring order, Gram blocks and coefficients keep their bits"""
    both = _scripted(3, ["aa", "aa"])
    st = both.st
    keep = [a.copy() for a in (st.h, st.order, st.conv, st.SS, st.SY, st.YY, st.delta)]
    both.move()
    f = both.f.copy()
    f[1, 2] = bad  # an atom of molecule 1
    st.sums(both.x, f)
    ret = st.control(both.step)
    assert ret[1] == O.UNUSABLE
    for a, k in zip((st.h, st.order, st.conv, st.SS, st.SY, st.YY, st.delta), keep):
        assert np.array_equal(a[1], k[1])


@pytest.mark.parametrize("longest,max_step,damping", [(0.1, 0.2, 1.0), (0.5, 0.2, 1.0), (0.25, 0.25, 1.0), (0.25, 0.25, 0.5),
                                                      (3.0, 0.2, 0.7), (1e-9, 0.2, 1.0)])
def test_clamp(longest, max_step, damping):
    """off, on, longest == max_step exactly, with damping: within 1 fp32 ulp of the oracle's"""
    p = dict(O.LBFGS, memory=1, max_step=max_step, damping=damping)
    st = H.State(np.zeros(1, np.int64), 1, p)
    st.conv[0] = -1
    st.direction[0] = [longest, 0, 0]
    st.longest2[0] = float(np.float32(longest)) ** 2
    x = st.move(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32))
    want = np.float32(O.clamp(st.direction.astype(np.float64), p))
    assert MO.ulp_distance(st.scale[0], want) <= 1
    assert x[0, 0] == np.float32(st.scale[0] * np.float32(longest))
    if longest == max_step:
        assert st.scale[0] == np.float32(damping)


# ---- 3. the wells -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memory", [1, 3, 100])
def test_wells_converge_in_both_precisions(memory):
    """1, 3, 40, 64 and 1 500 atoms, interleaved, a few fixed atoms: the header's fp32 run and the fp64 oracle both converge every
    molecule, the fp32 run in at most twice the oracle's steps (the cap catches a recursion that degenerates into clamped steepest
    descent)"""
    p = dict(P, memory=memory)
    batch, kspring, x0, x, fixed = _problem()
    for anh in (0.0, 2.0):
        n64, conv64, x64, _ = O.wells(batch, 5, kspring, x0, x, p, 1000, fixed, anharmonic=anh)
        n32, conv32, x32, h_log, acc_log = H.wells(batch, 5, kspring, x0, x, p, 1000, fixed, anharmonic=anh)
        print("memory", memory, "anharmonic", anh, "fp64", conv64.tolist(), "fp32", conv32.tolist())
        assert (conv64 >= 0).all() and (conv32 >= 0).all()
        assert (conv32 <= 2 * np.maximum(conv64, 1)).all()
        free = fixed == 0
        assert np.abs(kspring[:, None] * (x32 - x0))[free].max() < 2e-3
        assert np.array_equal(x32[~free], x[~free])
        assert h_log.max() <= memory


# ---- 4. the non-convex well ---------------------------------------------------------------------------------------------------------
def test_non_convex_well_rejects_the_same_pairs():
    """the quartic-softened well with anharmonicity 2.0 and memory 3: the oracle ITSELF (fp64, free running) rejects pairs, so the
    branch is exercised; the header then rejects the same pairs at the same steps as the oracle stepped along its trajectory (the
    comparison of every step is in _Both.control)"""
    p = dict(P, memory=3)
    batch, kspring, x0, x, fixed = _problem()
    n64, conv64, _, log = O.wells(batch, 5, kspring, x0, x, p, 1000, fixed, anharmonic=2.0)
    rejected64 = [(s, m) for s, (h, acc) in enumerate(log) for m in range(5) if 0 < s and (s < conv64[m]) and not acc[m]]
    assert len(rejected64) >= 1
    record = []
    both, steps = _wells_run(p, 2.0, 1000, record)
    conv = both.st.conv
    assert (conv >= 0).all()
    rejected32 = [(s, m) for s, (h, acc, c) in enumerate(record) for m in range(5) if 0 < s and s < conv[m] and not acc[m]]
    print("oracle rejects", len(rejected64), "header rejects", len(rejected32), rejected32[:8])
    assert rejected32 == rejected64  # (the free-running fp32 and fp64 runs reject the same pairs at the same steps)
    assert max(h.max() for h, _, _ in record) == 3  # the ring filled and wrapped


# ---- 5. the sanitizers --------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/lbfgs_host.hip with its own main, host code only (-Xarch_host -fsanitize=address,undefined): one non-convex well on heap
    arrays of exact size.  A report makes the program exit non-zero (-fno-sanitize-recover)."""
    exe = str(tmp_path / "lbfgs_host_san")
    subprocess.check_call([H.hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DLBFGS_HOST_MAIN", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", H.SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "steps" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


# ---- 6. signatures and exports ------------------------------------------------------------------------------------------------------
def test_header_and_bindings_declare_the_lbfgs_entries():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from torchmdnet_amd import _C

    src = open(_C.__file__).read()
    for name, n_args in (("tmdnet_lbfgs_workspace_bytes", 4), ("tmdnet_lbfgs_layout", 4), ("tmdnet_lbfgs_reset", 3),
                         ("tmdnet_lbfgs_advance", 26), ("tmdnet_lbfgs_status", 3)):
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == n_args, name
        assert name in _C.declared_symbols() and name + ".argtypes" in src


def test_library_exports_the_lbfgs_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10 and len(hip_lib.tmdnet_lbfgs_advance.argtypes) == 26
    nb = C.c_size_t(0)
    for n, b, mem in ((64, 1, 100), (5000, 2, 10), (300, 40, 3)):
        assert hip_lib.tmdnet_lbfgs_workspace_bytes(n, b, mem, C.byref(nb)) == 0
        assert nb.value >= 24 * (mem + 2) * n + b * 24 * (mem + 1) ** 2  # the documented size: per atom, per molecule
        off = (C.c_int64 * 17)()
        assert hip_lib.tmdnet_lbfgs_layout(n, b, mem, off) == 0
        assert list(off) == sorted(off) and off[0] == 0 and off[16] + 256 == nb.value and all(o % 256 == 0 for o in off)
    for n, b, mem in ((-1, 1, 3), (4, 1, 0), (4, 1, 513)):
        assert hip_lib.tmdnet_lbfgs_workspace_bytes(n, b, mem, C.byref(nb)) == 1
    # argument checks happen before anything is enqueued: no device is needed to be refused
    p = C.c_void_p(256)
    assert hip_lib.tmdnet_lbfgs_reset(None, None, 0) == 1
    assert hip_lib.tmdnet_lbfgs_status(None, None, (C.c_uint64 * 3)()) == 1
    args = [None, None, None, p, 4, 1, 2, p, p, None, None, None, None, p, 3, 70.0, 0.2, 1.0, 0.05] + [None] * 7
    for k, v in ((3, None), (7, None), (13, None), (14, 0), (15, 0.0), (16, -1.0), (17, 0.0), (18, 0.0), (6, 3), (5, 0)):
        bad = list(args)
        bad[k] = v
        assert hip_lib.tmdnet_lbfgs_advance(*bad) == 1, k


def test_capture_minimize_takes_lbfgs():
    from torchmdnet_amd import lbfgs
    from torchmdnet_amd.models.model import TorchMD_Net

    sig = inspect.signature(TorchMD_Net.capture_minimize).parameters
    assert "lbfgs" in sig and sig["lbfgs"].default is None
    assert lbfgs.parse_lbfgs({}) == dict(memory=100, alpha=70.0, max_step=0.2, damping=1.0) == lbfgs.LBFGS_DEFAULTS
    assert list(inspect.signature(lbfgs.DeviceLBFGS.reset).parameters)[1:] == ["pos"]


if __name__ == "__main__":
    got = measure()
    doc = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
    doc["gram_vs_two_loop"] = dict(
        what="max |p_header - p_two_loop| / max |p| in fp64 before the rounding to fp32: the coefficient-space recursion of "
             "tn_lbfgs_math.h (host build, one lane) against the two loops on the same stored pairs, CPU",
        cases=got, max=max(got.values()), test_bound_factor=64)
    steps = {}
    batch, kspring, x0, x, fixed = _problem()
    for memory in (1, 3, 100):
        for anh in (0.0, 2.0):
            p = dict(P, memory=memory)
            conv64 = O.wells(batch, 5, kspring, x0, x, p, 1000, fixed, anharmonic=anh)[1]
            conv32 = H.wells(batch, 5, kspring, x0, x, p, 1000, fixed, anharmonic=anh)[1]
            steps[f"memory_{memory}_anharmonic_{anh:g}"] = dict(fp64_oracle=conv64.tolist(), fp32_header=conv32.tolist())
    doc["wells_converged_at"] = dict(
        what="the step at which each well (1, 3, 40, 64, 1 500 atoms, interleaved, five fixed atoms, fmax 1e-3) converged: the float64 "
             "oracle free running, and the header's fp32 run on the CPU", runs=steps)
    json.dump(doc, open(PROFILE, "w"), indent=1)
    print(json.dumps(doc["gram_vs_two_loop"], indent=1), json.dumps(steps))
