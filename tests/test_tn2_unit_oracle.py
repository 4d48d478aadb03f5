"""Keeps tests/tn2_unit_oracle.py and tests/tn2_unit_cases.py honest without a device.

* the equilibration statement equals the corresponding lines of oracle/tn2_torch.charge_predict and the Coulomb statement equals
  oracle/tn2_torch.coulomb_per_atom (both pinned to the unmodified reference), in float64 to 1e-12, on the cases' own inputs;
* every adjoint statement (QEQ_BWD, CP_FEAT_BWD, g_q / fpos of the Coulomb head, the chain EDGE_GW -> EDGE_REDUCE -> PAIR_GD)
  equals torch.autograd.grad of its forward statement in float64 to 1e-10;
* EDGE_REVERSE equals a dictionary lookup on the hand-built graphs, which are in the engine's form;
* the constants restated in the cases module are the ones in csrc/tn_tn2.hip, and the case list AS A WHOLE has inputs on both
  sides of every boundary those constants make (the branch census), so a changed constant fails here instead of silently
  un-covering a branch of tests/test_gpu_tn2_unit.py;
* profiles/tn2_unit_floor.json has a bound by the project's rule for every output of every case.
"""
import os
import re

import pytest
import torch

from oracle import tn2_torch as T2
from tests import kernel_unit_cases as K
from tests import tn2_unit_cases as M
from tests import tn2_unit_oracle as O

TOL_PIN, TOL_GRAD = 1e-12, 1e-10
CSRC = os.path.join(M.ROOT, "torchmd-net_amd", "csrc")


def _rn(*s, seed=0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _f64(d):
    return M._to(d, lambda v: v.double())


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ====================================================================================== graphs
def test_graphs_are_in_the_engines_form():
    for name in M.GRAPHS:
        g = M.build_graph(name)
        N, P, rows, col, ep = g["N"], g["P"], g["rows"], g["col"], g["epair"]
        assert g["rowptr"][-1] == col.numel() == g["E"] == 2 * P + N
        assert torch.equal(rows, torch.repeat_interleave(torch.arange(N), g["rowptr"][1:] - g["rowptr"][:-1]))
        key = rows * N + col
        assert bool((key[1:] > key[:-1]).all())  # columns ascend within a row, no duplicates
        assert torch.equal(torch.sort(col * N + rows).values, key)  # symmetric
        self_e = rows == col
        assert int(self_e.sum()) == N and bool((ep[self_e] == P).all())
        assert bool((ep[~self_e] < P).all()) and torch.equal(torch.bincount(ep[~self_e], minlength=P), torch.full((P,), 2))
        assert bool((g["batch"][rows] == g["batch"][col]).all()) and bool((g["batch"][1:] >= g["batch"][:-1]).all())


def test_edge_reverse_is_a_dictionary_lookup():
    for name in M.GRAPHS:
        g = M.build_graph(name)
        where = {(int(i), int(j)): e for e, (i, j) in enumerate(zip(g["rows"], g["col"]))}
        erev, eid, pair_edge = O.edge_reverse(g)
        assert erev.tolist() == [where[(int(j), int(i))] for i, j in zip(g["rows"], g["col"])]
        assert eid.tolist() == list(range(g["E"]))
        want = [None] * g["P"]
        for (i, j), e in where.items():
            if j < i:
                want[int(g["epair"][e])] = e
        assert pair_edge.tolist() == want


# ====================================================================================== pinned to oracle/tn2_torch.py
@pytest.mark.parametrize("variant", M.QEQ_VARIANTS)
@pytest.mark.parametrize("qd", [3, 24])
def test_equilibration_is_the_oracles(monkeypatch, variant, qd):
    """charge_predict with its MLP replaced by the case's `out`: lines 40-45 of oracle/tn2_torch.py run as they are"""
    d = _f64(M.make_inputs(("qeq_fwd", variant, qd)))
    N, B = d["N"], d["B"]
    Q = None if variant == "noq" else d["Qmol"]
    monkeypatch.setattr(T2.TT, "lin", lambda x, sd, key, bias=True: d["out"] if key.endswith("q_mlp.layers.2") else x[:, :1])
    sd = {"p.q_norm.weight": torch.ones(6, dtype=torch.float64), "p.q_norm.bias": torch.zeros(6, dtype=torch.float64)}
    Qatom = torch.zeros(N, dtype=torch.float64) if Q is None else Q[d["batch"]]
    want = T2.charge_predict(sd, "p.", _rn(N, 3, 3, 2, seed=1), d["batch"], Qatom, B, qd)
    got, Fu, dQ = O.qeq_fwd(d["out"], Q, d["batch"], B, qd)
    assert O.group_rel_err(got, want, d["batch"]) < TOL_PIN
    assert bool((Fu > 0).all()) and Fu.shape == dQ.shape == (B, qd)
    # permuted atoms: the same answer after un-permuting (what the counts[3] = 1 cases of the device test rely on)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(qd))
    gp, Fup, dQp = O.qeq_fwd(d["out"][perm], Q, d["batch"][perm], B, qd)
    assert O.group_rel_err(gp, got[perm], d["batch"][perm]) < TOL_PIN and _rel(Fup, Fu) < TOL_PIN and _rel(dQp, dQ) < TOL_PIN


@pytest.mark.parametrize("mode", M.COULOMB_MODES)
def test_coulomb_energy_is_the_oracles(mode):
    for QC in (1, 9):
        d = _f64(M.make_inputs(("coulomb", mode + "-sorted", QC)))
        n = d["N"] - 1  # the oracle has no atom outside every molecule
        hp = dict(coulomb_cutoff=None if mode == "a2a" else M.COULOMB_CUT, coulomb_epsilon_solvent=M.COULOMB_EPS)
        box = None if d["box"] is None else (d["box"][0] if d["box_mode"] == 1 else d["box"])
        want = T2.coulomb_per_atom(hp, d["charges"][:n], d["pos"][:n], d["batch"][:n], d["wq"], box)
        args = lambda s: (d["pos"][s], d["batch"][s], d["B"], d["box"], d["box_mode"], d["charges"][s], d["wq"], d["cut"], M.COULOMB_EPS, M.COULOMB_SCALE)
        got = O.coulomb(*args(slice(0, n)), want_grad=False)["ec"]
        assert O.group_rel_err(got, want, d["batch"][:n]) < TOL_PIN, (mode, QC)
        assert float(want.abs().max()) > 1e-3
        # the atom outside every molecule: energy 0, nobody else's energy changes; and a permutation permutes the result
        full = O.coulomb(*args(slice(None)))
        assert float(full["ec"][n]) == 0 and float(full["g_q"][n].abs().max()) == 0 and float(full["fpos"][n].abs().max()) == 0
        assert O.group_rel_err(full["ec"][:n], want, d["batch"][:n]) < TOL_PIN
        perm = torch.randperm(d["N"], generator=torch.Generator().manual_seed(3))
        for k, v in O.coulomb(*args(perm)).items():
            assert O.group_rel_err(v, full[k][perm], d["batch"][perm].clamp(max=d["B"])) < TOL_PIN, (mode, QC, k)


# ====================================================================================== adjoints against autograd
def test_cp_feat_and_its_adjoint():
    X = _rn(7, 9, 5, seed=2).requires_grad_()
    g_feat = _rn(7, 3, 5, seed=3)
    feat = O.cp_feat(X)
    u = X.detach()
    t = u[:, 4] + u[:, 7]
    assert _rel(feat[:, 0].detach(), u[:, 0]) < TOL_PIN  # I = trace / 3 is the stored component 0
    assert _rel(feat[:, 1].detach(), 2 * (u[:, 1:4] ** 2).sum(1)) < TOL_PIN
    assert _rel(feat[:, 2].detach(), u[:, 4] ** 2 + u[:, 7] ** 2 + t * t + 2 * (u[:, 5] ** 2 + u[:, 6] ** 2 + u[:, 8] ** 2)) < TOL_PIN
    (auto,) = torch.autograd.grad((g_feat * feat).sum(), X)
    assert O.group_rel_err(O.cp_feat_bwd(u, g_feat), auto) < TOL_GRAD


@pytest.mark.parametrize("variant", M.QEQ_VARIANTS)
@pytest.mark.parametrize("qd", M.QEQ_QD)
def test_qeq_adjoint_is_autograd(variant, qd):
    d = _f64(M.make_inputs(("qeq_bwd", variant, qd)))
    out = d["out"].clone().requires_grad_()
    Q = None if variant == "noq" else d["Qmol"]
    c, Fu, dQ = O.qeq_fwd(out, Q, d["batch"], d["B"], qd)
    (auto,) = torch.autograd.grad((d["g_c"] * c).sum(), out)
    got = O.qeq_bwd(d["out"], Fu.detach(), dQ.detach(), d["g_c"], d["batch"], qd)
    assert O.group_rel_err(got, auto, d["batch"]) < TOL_GRAD
    if variant == "neutral":  # the + 1e-6 matters: it is a tenth or more of Fu in every molecule
        assert float((1e-6 / Fu.detach()).min()) > 0.1


@pytest.mark.parametrize("mode", M.COULOMB_MODES)
def test_coulomb_gradients_are_autograd(mode):
    d = _f64(M.make_inputs(("coulomb", mode + "-sorted", 9)))
    pos, q = d["pos"].clone().requires_grad_(), d["charges"].clone().requires_grad_()
    args = (d["batch"], d["B"], d["box"], d["box_mode"])
    e = O.coulomb(pos, *args, q, d["wq"], d["cut"], M.COULOMB_EPS, M.COULOMB_SCALE, want_grad=False)["ec"]
    gp, gq = torch.autograd.grad(M.COULOMB_SCALE * e.sum(), [pos, q])
    got = O.coulomb(d["pos"], *args, d["charges"], d["wq"], d["cut"], M.COULOMB_EPS, M.COULOMB_SCALE)
    grp = d["batch"].clamp(max=d["B"])
    assert O.group_rel_err(got["g_q"], gq, grp) < TOL_GRAD and O.group_rel_err(got["fpos"], -gp, grp) < TOL_GRAD


@pytest.mark.parametrize("gname", sorted(M.GRAPHS))
def test_edge_chain_adjoints_are_autograd(gname):
    """L = sum(gMi * M(w)), w = silu(pre3) Ce, pre3 = he1 W3 (any per-edge map stands for the layers between), pre1 = Ap[p] + Bt[i]
    + Cs[j], Ap = Ap0 + d dAp and C = C0 + d dC per pair: EDGE_GW gives dL/dpre3 and dL/dCe, EDGE_REDUCE dL/dBt, dL/dCs, dL/dAp,
    PAIR_GD dL/dd."""
    g = M.build_graph(gname)
    N, P, E, F = g["N"], g["P"], g["E"], 70  # two slot arrays, the second partial
    Ap0, dAp, C0, dC = (_rn(P + 1, F, seed=4).requires_grad_(), _rn(P + 1, F, seed=5), torch.rand(P + 1, dtype=torch.float64).requires_grad_(),
                        _rn(P + 1, seed=6))
    Bt, Cs, W3 = _rn(N, F, seed=7).requires_grad_(), _rn(N, F, seed=8).requires_grad_(), _rn(F, 3 * F, seed=9) / F ** 0.5
    gMi, Pn = _rn(N, 9, F, seed=10), _rn(N, 9, F, seed=11)
    dd = torch.zeros(P, dtype=torch.float64, requires_grad=True)
    d1 = torch.cat([dd, torch.zeros(1, dtype=torch.float64)])
    pre1, he1, Ce = O.edge_pre1(g, Ap0 + d1[:, None] * dAp, Bt, Cs, C0 + d1 * dC)
    assert torch.equal(he1, O.silu(pre1)) and torch.equal(Ce.detach(), C0.detach()[g["epair"]])
    pre3 = he1 @ W3
    L = (gMi * O.edge_message(g, pre3, Ce, Pn)).sum()
    a_pre3, a_Bt, a_Cs, a_Ap, a_C, a_d = torch.autograd.grad(L, [pre3, Bt, Cs, Ap0, C0, dd])
    g_pre3, slots, scale = O.edge_gw(g, gMi, Pn, pre3.detach(), Ce.detach())
    assert slots.shape == scale.shape == (2, E) and bool((scale > 0).all())
    assert O.group_rel_err(g_pre3, a_pre3) < TOL_GRAD
    g_C = torch.zeros(P + 1, dtype=torch.float64).index_add(0, g["epair"], slots.sum(0))
    assert float((g_C - a_C).abs().max()) < TOL_GRAD * float(scale.sum(0).max())
    g_pre1 = (g_pre3 @ W3.t()) * O.silu_grad(pre1.detach())
    gB, gCs, gAp = O.edge_reduce(g, g_pre1)
    assert O.group_rel_err(gB, a_Bt) < TOL_GRAD and O.group_rel_err(gCs, a_Cs) < TOL_GRAD and O.group_rel_err(gAp, a_Ap[:P]) < TOL_GRAD
    gd = O.pair_gd(g, gAp, dAp, slots, dC)
    assert float((gd - a_d).abs().max()) < TOL_GRAD * float(a_d.abs().max())


# ====================================================================================== constants and the branch census
def test_constants_restated_in_the_cases_are_the_sources():
    src = open(os.path.join(CSRC, "tn_tn2.hip")).read()
    ints = lambda pat: [tuple(int(v) for v in (m if isinstance(m, tuple) else (m,))) for m in re.findall(pat, src)]
    assert ints(r"for \(int base = j0; base < j1; base \+= (\d+)\)") == [(M.COULOMB_ROUND,)]
    assert ints(r"__shared__ float red\[2\]\[(\d+)\]") == [(M.QEQ_BLOCK,)] and ints(r"const int groups = (\d+) / qd") == [(M.QEQ_BLOCK,)]
    assert ints(r"\(k_qeq<(?:false|true)>\), dim3\(B\), dim3\((\d+)\)") == [(M.QEQ_BLOCK,)] * 2
    assert ints(r"for \(; e \+ (\d+) <= e1; e \+= (\d+)\)") == [(M.EDGE_TRIP, M.EDGE_TRIP)] * 3  # pre1, gw, reduce
    assert ints(r"dim3\(t > (\d+) \? (\d+) : t\)") == [(M.ROW_THREADS_CAP, M.ROW_THREADS_CAP)] * 2  # pre1, reduce
    assert ints(r"int tn2_gw_slots\(int F\) \{ return \(F \+ (\d+)\) / (\d+); \}") == [(M.WAVE - 1, M.WAVE)] and O.WAVE == M.WAVE
    assert "(lane & 15) == 0" in src and "e + (lane >> 4)" in src and M.WAVE // 16 == M.EDGE_TRIP  # one lane per edge of a trip
    assert len(ints(r"blockIdx\.x \* (\d+) \+ \(threadIdx\.x >> 6\)")) == 4 and set(ints(r"blockIdx\.x \* (\d+) \+ \(threadIdx\.x >> 6\)")) == {(M.ATOMS_PER_BLOCK,)}
    assert ints(r"constexpr int kMaxQC = (\d+);") == [(M.MAX_QC,)]
    assert "1.0f / 4.6f" in src and O.R_DAMP == 4.6 and "1.0e-6f" in src
    assert K.SENTINEL == 0x7FC0BEEF and K.TAIL == 64


def test_case_list_has_both_sides_of_every_boundary():
    cases = M.all_cases()
    ops = {c[0] for c in cases}
    assert ops == set(M.OPS) and len({M.case_id(c) for c in cases}) == len(cases)
    # ---- k_coulomb: lanes walk a molecule in rounds; a wave per atom, four per block; channel chunks of 8 with a k < QC guard
    R, sizes = M.COULOMB_ROUND, M.COULOMB_SIZES
    assert {1, 2, R - 1, R, R + 1} <= set(sizes) and any(n > 2 * R and n % R for n in sizes)  # a third, partial round
    assert (sum(sizes) + 1) % M.ATOMS_PER_BLOCK  # partial last block
    qcs = M.COULOMB_QC
    assert 1 in qcs and 8 in qcs and 9 in qcs and any(q > 16 and q % 8 == 0 and q < M.MAX_QC for q in qcs) and M.MAX_QC in qcs
    want = {("coulomb", f"{m}-{o}", q) for m in M.COULOMB_MODES for o in M.COULOMB_ORDERS for q in qcs}
    assert want <= set(cases)
    for mode in M.COULOMB_MODES:
        geo = M.coulomb_geometry(mode)  # its builder asserted the conditions on the positions
        assert geo["N"] == sum(sizes) + 1 and int(geo["batch"][-1]) == geo["B"] and (geo["cut"] > 0) == (mode != "a2a")
        assert geo["box_mode"] == {"a2a": 0, "rf": 0, "rf_box": 1, "rf_molbox": 2}[mode]
        if geo["box_mode"]:
            assert bool((geo["box"][:, 1, 0].abs() > 0).all()) and geo["box"].shape[0] == (1 if geo["box_mode"] == 1 else geo["B"])
            d = M.make_inputs(("coulomb", mode + "-sorted", 1))
            _, delta, _ = O.coulomb_table(d["pos"].double(), d["batch"], d["B"], d["box"].double(), d["box_mode"], d["cut"])
            plain = d["pos"].double()[:, None] - d["pos"].double()[None, :]
            assert bool(((delta - plain).abs() > 1).any())  # some pair really takes an image
    d = M.make_inputs(("coulomb", "rf-perm", 9))
    assert d["unsorted"] == 1 and bool((d["batch"][1:] < d["batch"][:-1]).any())
    # ---- k_qeq: 256 / qd groups per molecule, dead threads when qd does not divide the block
    assert {M.QEQ_BLOCK % qd for qd in M.QEQ_QD} >= {0, 1, 16} and 1 in M.QEQ_QD and M.MAX_QC in M.QEQ_QD
    for qd in M.QEQ_QD:
        groups = M.QEQ_BLOCK // qd
        assert set(M.qeq_sizes(qd)) == {groups - 1, groups, groups + 1, 1}
        assert {("qeq_fwd", v, qd) for v in M.QEQ_VARIANTS} | {("qeq_bwd", v, qd) for v in M.QEQ_VARIANTS} <= set(cases)
    # ---- edge kernels: trips of four edges and a tail; lanes 0, 16, 32, 48 write a trip's sums; channel loop above the thread cap
    T = M.EDGE_TRIP
    lens = set(M.row_lengths("rows"))
    assert set(range(1, T + 2)) | {2 * T, 2 * T + 1} <= lens and 1 in M.row_lengths("two_mols")
    assert all(M.build_graph(n)["N"] % M.ATOMS_PER_BLOCK for n in M.GRAPHS) and M.build_graph("rows")["N"] <= 24
    assert all((M.build_graph(n)["P"] + M.PAIR_CAP_EXTRA) % M.ATOMS_PER_BLOCK for n in M.GRAPHS)  # k_tn2_pair_gd: partial last block
    Fs, W, cap = M.EDGE_F, M.WAVE, M.ROW_THREADS_CAP
    assert any(F < W for F in Fs) and any(W < F < 2 * W for F in Fs) and any(F % W == 0 and F <= cap for F in Fs)
    assert any(F > cap and F % cap for F in Fs) and {(F + W - 1) // W for F in Fs} >= {1, 2, 5}
    assert {(op, n, F) for op in M.EDGE_OPS for n in M.GRAPHS for F in Fs} <= set(cases)
    assert {("cp_feat", "rows", F) for F in M.CP_F} <= set(cases) and any(F % W for F in M.CP_F)
    assert (M.GRAPHS["rows"][0] * min(M.CP_F)) % 256  # k_cp_feat: partial last block


# ====================================================================================== the floor file
def test_floor_file_has_a_bound_by_the_rule_for_every_case():
    doc = M.load_bounds()["cases"]
    assert set(doc) == {M.case_id(c) for c in M.all_cases()}
    for case in M.all_cases():
        ent = doc[M.case_id(case)]
        assert set(ent) == set(M.OUTPUTS[case[0]])
        for k, v in ent.items():
            if k in M.EXACT:
                assert v["floor"] == 0 and v["bound"] == 0
            else:
                assert v["bound"] == K.bound_of(v["floor"]) and K.BOUND_MIN <= v["bound"] <= K.BOUND_CAP


def test_floor_file_matches_a_recomputed_floor():
    """two small cases recomputed: the file belongs to these inputs"""
    for case in (("edge_gw", "two_mols", 96), ("coulomb", "rf_box-perm", 9)):
        ent = M.load_bounds()["cases"][M.case_id(case)]
        for k, e in M.floor_of(case).items():
            assert 0.5 * ent[k]["floor"] <= e <= 2 * ent[k]["floor"], (k, e, ent[k]["floor"])
