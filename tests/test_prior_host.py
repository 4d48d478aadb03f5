"""The ZBL / D2 pair priors without a GPU: the header's pair arithmetic (csrc/tn_prior_math.h, compiled host-only by
tests/prior_host_mirror.py) against the float64 statement tests/prior_oracle.py; the oracle against its own finite differences and
against the unmodified reference (tests/golden/priors_ref.pt, tools/make_golden_priors.py); the Python surface (create_model,
state-dict keys, load_model, refusals) and the C ABI's declarations.

Bound of the fp32 pair arithmetic: 1e-5 (the project's golden-vector tolerance) times the sum of the absolute terms the value is made
of - the terms cancel (the cosine cutoff is 1/2 cos + 1/2, D2's slope is a difference), so the value itself is not the scale.
About twenty fp32 roundings and four expf per pair: about 1e-6 is expected."""
import os
import re

import numpy as np
import pytest
import torch

from tests import prior_host_mirror as H
from tests import prior_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, HARTREE, EV = 1e-10, 4.3597447222071e-18, 1.602176634e-19
PAIRS = {"H-H": (1, 1), "C-O": (6, 8), "I-Xe": (53, 54)}


def d2_table():
    from torchmdnet_amd.priors import D2

    t = D2.C_6_R_r.double().numpy()
    return t[:, 0], t[:, 1]


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return torch.load(os.path.join(golden_dir, "priors_ref.pt"), weights_only=False)


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("cutoff,es", [(5.0, EV), (3.0, HARTREE)])
def test_zbl_pair_against_oracle(pair, cutoff, es):
    Zi, Zj = PAIRS[pair]
    r = np.linspace(0.3, cutoff, 400, endpoint=False).astype(np.float32)
    u, du = H.zbl(r, Zi, Zj, cutoff, A, es)
    r64 = r.astype(np.float64)
    uo, duo = O.zbl_u(r64, Zi, Zj, cutoff, A, es), O.zbl_u(r64, Zi, Zj, cutoff, A, es, deriv=1)
    # absolute terms: u = pre phi (1/2 cos + 1/2) / r;  u' = pre [phi' C + phi C' - phi C / r] / r
    s = A / (0.8854 * O.BOHR / (Zi ** 0.23 + Zj ** 0.23))
    phi = sum(c * np.exp(-k * r64 * s) for c, k in O.ZBL_C)
    dphi = sum(c * k * s * np.exp(-k * r64 * s) for c, k in O.ZBL_C)
    pre = O.ZBL_E / es / A * Zi * Zj
    S_u = pre * phi / r64
    S_du = pre * (dphi + phi * 0.5 * np.pi / cutoff + phi / r64) / r64
    worst = max((np.abs(u - uo) / S_u).max(), (np.abs(du - duo) / S_du).max())
    print(f"zbl {pair} cutoff {cutoff}: worst |host - oracle| / S = {worst:.2e}")
    assert worst <= 1e-5


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_d2_pair_against_oracle(pair):
    Zi, Zj = PAIRS[pair]
    C6, Rr = d2_table()
    cutoff = 10.0
    r = np.linspace(0.3, cutoff, 400, endpoint=False).astype(np.float32)
    u, du = H.d2(r, C6[Zi], C6[Zj], Rr[Zi], Rr[Zj], cutoff, A, EV)
    r64 = r.astype(np.float64)
    args = (C6[Zi], C6[Zj], Rr[Zi], Rr[Zj], A, EV)
    uo, duo = O.d2_u(r64, *args), O.d2_u(r64, *args, deriv=1)
    # u' = pre [f' / R^6 - 6 f / R^7] snm: the two terms have opposite signs
    R, rr = r64 * 0.1, Rr[Zi] + Rr[Zj]
    t = np.exp(-20.0 * (R / rr - 1.0))
    f = 1.0 / (1.0 + t)
    pre = np.sqrt(C6[Zi] * C6[Zj]) / (EV * O.AVOGADRO)
    S_du = pre * (20.0 / rr * t * f * f / R ** 6 + 6.0 * f / R ** 7) * 0.1
    worst = max((np.abs(u - uo) / np.abs(uo)).max(), (np.abs(du - duo) / S_du).max())
    print(f"d2 {pair}: worst |host - oracle| / S = {worst:.2e}")
    assert worst <= 1e-5


def test_pair_test_and_limit():
    assert H.in_cutoff(1.0, 2.0) and not H.in_cutoff(4.0, 2.0) and not H.in_cutoff(0.0, 2.0)
    from torchmdnet_amd import _C, priors

    assert H.max_molecule_atoms() == priors.MAX_MOLECULE_ATOMS == _C.PRIOR_MAX_MOLECULE_ATOMS == 32768
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_PRIOR_MAX_MOLECULE_ATOMS\s+32768\b", txt)


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_oracle_slope_against_central_difference(pair):
    Zi, Zj = PAIRS[pair]
    C6, Rr = d2_table()
    r = np.linspace(0.3, 4.9, 200).astype(np.longdouble)
    h = np.longdouble(1e-6)
    for u, args in ((O.zbl_u, (Zi, Zj, 5.0, A, EV)), (O.d2_u, (C6[Zi], C6[Zj], Rr[Zi], Rr[Zj], A, EV))):
        fd = (u(r + h, *args) - u(r - h, *args)) / (2 * h)
        an = u(r, *args, deriv=1)
        # truncation h^2 u''' / 6 with u''' / u' < 1e4 on this range: under 2e-9 relative; rounding of the quotient far below
        assert (np.abs(fd - an) / np.abs(an).max()).max() < 1e-7


def _cluster(seed, n, spread):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 19, n), rng.normal(size=(n, 3)) * spread


def test_oracle_virial_against_strain_difference(golden_dir):
    C6, Rr = d2_table()
    spec = np.arange(20)
    zbl = dict(cutoff=4.0, distance_scale=A, energy_scale=EV, Z=spec.astype(float))
    d2 = dict(cutoff=6.0, distance_scale=A, energy_scale=EV, C6=C6[spec], Rr=Rr[spec])
    box = torch.load(os.path.join(golden_dir, "tiny_pbc_ref.pt"))["box"].double().numpy()
    z, pos = _cluster(5, 24, 2.5)
    batch = np.zeros(24, int)
    for b in (None, box):
        ref = O.evaluate(pos, z, batch, 1, b, zbl, d2)
        assert ref["margin"] > 1e-4
        h = 1e-6
        for a in range(3):
            for c in range(3):
                eps = np.zeros((3, 3))
                eps[a, c] = h
                Ep = O.energy_only(pos @ (np.eye(3) + eps), z, batch, 1, None if b is None else b @ (np.eye(3) + eps), zbl, d2)
                Em = O.energy_only(pos @ (np.eye(3) - eps), z, batch, 1, None if b is None else b @ (np.eye(3) - eps), zbl, d2)
                fd = -(Ep - Em)[0] / (2 * h)
                assert abs(fd - ref["W"][0, a, c]) <= 1e-6 * ref["S_W"][0, a, c] + 1e-9, (a, c, fd, ref["W"][0, a, c])
        # and the forces against a displacement of one atom
        for i in (0, 7):
            for c in range(3):
                d = np.zeros_like(pos)
                d[i, c] = h
                fd = -(O.energy_only(pos + d, z, batch, 1, b, zbl, d2) - O.energy_only(pos - d, z, batch, 1, b, zbl, d2))[0] / (2 * h)
                assert abs(fd - ref["F"][i, c]) <= 1e-6 * ref["S_F"][i, c] + 1e-9


def oracle_priors(settings_name, fixture):
    """The oracle's prior dicts of one fixture setting."""
    C6, Rr = d2_table()
    pm, pa = fixture["settings"][settings_name]
    names = [pm] if isinstance(pm, str) else list(pm or [])
    zbl = d2 = None
    for name, a in zip(names, pa or []):
        an = np.asarray(a.get("atomic_number", []))
        if name == "ZBL":
            zbl = dict(cutoff=a["cutoff_distance"], distance_scale=a["distance_scale"], energy_scale=a["energy_scale"], Z=an.astype(float))
        elif name == "D2":
            d2 = dict(cutoff=a["cutoff_distance"], distance_scale=a["distance_scale"], energy_scale=a["energy_scale"], C6=C6[an], Rr=Rr[an])
    return zbl, d2, "Atomref" in names


@pytest.mark.parametrize("arch", ["tensornet", "equivariant-transformer"])
@pytest.mark.parametrize("setting", ["ZBL", "D2", "Atomref+ZBL+D2"])
def test_oracle_against_reference_fixture(fixture, arch, setting):
    """Prior-only energies of the reference = its with-prior minus its without-prior prediction (two fp32 numbers: their difference
    carries the rounding of both, eps32 each, on top of the fp32 pair sums' 1e-5 S)."""
    res = fixture["cases"][arch]["results"]
    zbl, d2, atomref = oracle_priors(setting, fixture)
    z, pos, batch, n_mol = fixture["z"].numpy(), fixture["pos"].numpy(), fixture["batch"].numpy(), fixture["n_mol"]
    want = O.evaluate(pos, z, batch, n_mol, None, zbl, d2)
    assert want["margin"] > 1e-4
    E = want["E"].copy()
    S = want["S_E"].copy()
    if atomref:
        ar = np.zeros(n_mol)
        np.add.at(ar, batch, fixture["atomref"].double().numpy()[z, 0])
        E += ar
        np.add.at(S, batch, np.abs(fixture["atomref"].double().numpy()[z, 0]))
    y1, y0 = res[setting]["y"].double().numpy()[:, 0], res["none"]["y"].double().numpy()[:, 0]
    eps = np.finfo(np.float32).eps
    bound = 1e-5 * S + 4 * eps * (np.abs(y1) + np.abs(y0))
    assert (np.abs((y1 - y0) - E) <= bound).all(), (y1 - y0, E, bound)
    assert (np.abs(E[[0, 3, 4]]) > 1e-4).all() and E[2] == 0.0  # the priors are visible; the empty molecule gets nothing
    if setting == "ZBL":  # and in the triclinic box
        p = fixture["pbc"]
        w = O.evaluate(p["pos"].numpy(), p["z"].numpy(), p["batch"].numpy(), 1, p["box"].double().numpy(), zbl, None)
        assert w["margin"] > 1e-4
        y1, y0 = res["ZBL"]["y_pbc"].double().numpy()[:, 0], res["none"]["y_pbc"].double().numpy()[:, 0]
        assert (np.abs((y1 - y0) - w["E"]) <= 1e-5 * w["S_E"] + 4 * eps * (np.abs(y1) + np.abs(y0))).all()
        wo = O.evaluate(p["pos"].numpy(), p["z"].numpy(), p["batch"].numpy(), 1, None, zbl, None)
        assert abs(wo["E"][0] - w["E"][0]) > 1e-3 * abs(w["E"][0])  # the box matters in this fixture


def _args(fixture, arch, pm, pa=None):
    return dict(fixture["cases"][arch]["args"], prior_model=pm, prior_args=pa)


def test_create_model_accepts_every_spelling(fixture):
    """(fails on a build without the priors: create_prior_models raised NotImplementedError for ZBL)"""
    from torchmdnet_amd import priors
    from torchmdnet_amd.models.model import create_model

    assert priors.__all__ == ["Atomref", "D2", "ZBL"]
    _, (zbl_args,) = fixture["settings"]["ZBL"]
    _, (d2_args,) = fixture["settings"]["D2"]
    spellings = [("ZBL", zbl_args), ("ZBL", [zbl_args]), (["ZBL", "D2"], [zbl_args, d2_args]), ([{"ZBL": zbl_args}, {"D2": d2_args}], None),
                 ({"D2": d2_args}, None)]
    for pm, pa in spellings:
        m = create_model(_args(fixture, "tensornet", pm, pa))
        kinds = [type(p).__name__ for p in m.prior_model]
        want = [pm] if isinstance(pm, str) else [next(iter(x)) if isinstance(x, dict) else x for x in (pm if isinstance(pm, list) else [pm])]
        assert kinds == want
        for p in m.prior_model:
            a = p.get_init_args()
            ref = zbl_args if isinstance(p, priors.ZBL) else d2_args
            assert a["atomic_number"] == ref["atomic_number"] and a["max_num_neighbors"] == ref["max_num_neighbors"]
            assert a["cutoff_distance"] == ref["cutoff_distance"] and a["distance_scale"] == pytest.approx(ref["distance_scale"], rel=1e-6)
            assert type(p)(**a).get_init_args() == a
            with pytest.raises(NotImplementedError, match="parameter container"):
                p.post_reduce(None, None, None, None)

    class Dataset:  # the dataset= fallback of both classes
        atomic_number, distance_scale, energy_scale = zbl_args["atomic_number"], 1e-10, EV

    for cls in (priors.ZBL, priors.D2):
        p = cls(5.0, 32, dataset=Dataset())
        assert p.get_init_args()["energy_scale"] == pytest.approx(EV, rel=1e-6) and p.get_init_args()["atomic_number"] == Dataset.atomic_number


@pytest.mark.parametrize("arch", ["tensornet", "equivariant-transformer"])
@pytest.mark.parametrize("setting", ["ZBL", "D2", "Atomref+ZBL+D2"])
def test_state_dict_keys_are_the_references(fixture, arch, setting):
    from torchmdnet_amd.models.model import create_model

    pm, pa = fixture["settings"][setting]
    m = create_model(_args(fixture, arch, pm, pa))
    assert sorted(m.state_dict().keys()) == fixture["cases"][arch]["results"][setting]["keys"]


def test_load_model_of_a_reference_checkpoint(fixture, tmp_path):
    from torchmdnet_amd import priors
    from torchmdnet_amd.models.model import load_model

    setting = "Atomref+ZBL+D2"
    pm, pa = fixture["settings"][setting]
    sd = fixture["cases"]["tensornet"]["results"][setting]["state_dict"]
    path = str(tmp_path / "priors.ckpt")
    torch.save(dict(hyper_parameters=_args(fixture, "tensornet", pm, pa), state_dict={"model." + k: v for k, v in sd.items()}), path)
    m = load_model(path)  # strict
    assert [type(p) for p in m.prior_model] == [priors.Atomref, priors.ZBL, priors.D2]
    for k, v in m.state_dict().items():
        assert v.dtype == sd[k].dtype and torch.allclose(v, sd[k], rtol=0, atol=0, equal_nan=True), k  # (row 0 of the D2 table is NaN)
    zbl, d2 = m._pair_priors()
    assert zbl.atomic_number.tolist() == pa[1]["atomic_number"] and torch.equal(d2.C_6[1:], priors.D2.C_6_R_r[1:, 0].float())


def test_refusals(fixture):
    from torchmdnet_amd import priors
    from torchmdnet_amd.models.model import create_model

    _, (zbl_args,) = fixture["settings"]["ZBL"]
    _, (d2_args,) = fixture["settings"]["D2"]
    with pytest.raises(NotImplementedError, match="Coulomb.*partial_charges"):
        create_model(_args(fixture, "tensornet", "Coulomb", dict(lower_switch_distance=1.0, upper_switch_distance=2.0, max_num_neighbors=32)))
    with pytest.raises(NotImplementedError, match="several ZBL"):
        create_model(_args(fixture, "tensornet", ["ZBL", "ZBL"], [zbl_args, zbl_args]))
    with pytest.raises(NotImplementedError, match="several D2"):
        create_model(_args(fixture, "tensornet", ["D2", "D2"], [d2_args, d2_args]))
    # a species without a C6 / R_r row: element 0, and an element beyond Xe
    d2 = priors.D2(**dict(d2_args, atomic_number=[0, 1, 6, 60]))
    d2.check_species(torch.tensor([1, 2, 2, 1]))
    with pytest.raises(NotImplementedError, match=r"species \[0\]"):
        d2.check_species(torch.tensor([1, 0, 2]))
    with pytest.raises(NotImplementedError, match=r"species \[3\]"):
        d2.check_species(torch.tensor([3]))
    sq, rr = d2.species_tables(6)
    assert np.isnan(sq[[0, 3, 4, 5]]).all() and np.isfinite(sq[[1, 2]]).all() and rr[1] == np.float32(0.1001)
    # the brute-force limit, on the host: nothing that large is allocated
    priors.check_molecule_size(32768)
    with pytest.raises(NotImplementedError, match="32768.*cell-list"):
        priors.check_molecule_size(32769)
    m = create_model(_args(fixture, "tensornet", ["ZBL", "D2"], [zbl_args, d2_args]))
    for what in ("atom weights", "hessian"):
        with pytest.raises(NotImplementedError, match="pair priors have no HIP path"):
            m._refuse_pair_priors(what)
    create_model(_args(fixture, "tensornet", None))._refuse_pair_priors("anything")  # a prior-free model refuses nothing
    # the fingerprint sees a changed prior argument (a stale captured graph then raises, tests/test_gpu_priors.py)
    fp = m._fingerprint()
    m.prior_model[0].cutoff_distance = 3.5
    assert m._fingerprint() != fp
    # property heads drop the priors, as before
    with pytest.warns(UserWarning, match="Dropping the prior model"):
        assert create_model(dict(_args(fixture, "tensornet", "ZBL", zbl_args), output_model="DipoleMoment", derivative=False)).prior_model is None


def test_header_and_bindings_are_additive(hip_lib):
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from torchmdnet_amd import _C

    src = open(_C.__file__).read()
    for name, n in (("tmdnet_set_pair_priors", 2), ("tmdnet_pair_priors_workspace_bytes", 4), ("tmdnet_pair_priors_add", 15),
                    ("tmdnet_debug_prior", 15)):
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == n, name
        assert name in _C.declared_symbols() and name + ".argtypes" in src
        assert len(getattr(hip_lib, name).argtypes) == n and hasattr(hip_lib, name)
    # the struct of the binding has the header's fields, in order
    body = re.search(r"typedef struct \{([^}]*)\} tmdnet_pair_priors;", code, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*[;,]", body)
    assert fields == [n for n, _ in _C.PairPriors._fields_]
    # without a device the entry still refuses what it must: NULL clears, atom weights are invalid
    assert hip_lib.tmdnet_set_pair_priors(None, None) == _C.ERR_INVALID
