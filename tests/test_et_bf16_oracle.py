"""No GPU: the rounding-aware mode of the ET oracle (oracle/et_torch.py, ``pair_rows="bf16"``: what the engine computes with
``pair_storage="bf16"``), the noise floor and the power of the bound the GPU tests take from it (oracle/et_bf16_floor.py,
profiles/et_bf16_oracle_floor.json), and the spellings of the pair-row modes in the bindings."""
import json
import os
import re

import pytest
import torch

from oracle import et_bf16_floor as B
from oracle import et_torch as ET
from torchmdnet_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


def _tiny(di, seed=3):
    """(state dict fp64, hp, z, pos fp64, batch) of a two-layer model with the given distance influence: two ragged molecules."""
    from torchmdnet_amd.models.model import create_model

    args = dict(W.ET_TINY_ARGS, distance_influence=di, cutoff_upper=5.0)
    torch.manual_seed(seed)
    sd = B.f64({k: v.detach() for k, v in create_model(dict(args)).state_dict().items()})
    za, pa, _ = W.synthetic_batch(n_mol=1, n_atoms=11, first_seed=70)
    zb, pb, _ = W.synthetic_batch(n_mol=1, n_atoms=7, first_seed=71)
    z, pos = torch.cat([za, zb]) % 19 + 1, torch.cat([pa, pb]).double()
    batch = torch.cat([torch.zeros(11, dtype=torch.long), torch.ones(7, dtype=torch.long)])
    return sd, ET.hparams_from_args(args), z, pos, batch


@pytest.mark.parametrize("di", ["both", "keys", "values"])
def test_identity_rounding_equals_the_plain_oracle(di):
    """the forward-mode tangent and the value + tangent recombination, without any rounding: E and F of the existing oracle"""
    sd, hp, z, pos, batch = _tiny(di)
    E0, F0 = ET.energy_and_forces(sd, hp, z, pos, batch)
    E1, F1 = ET.energy_and_forces(sd, hp, z, pos, batch, pair_rows=lambda x: x)
    assert rel(E1, E0) < 1e-12 and rel(F1, F0) < 1e-12
    Ed, Fd = ET.energy_and_forces(sd, hp, z, pos, batch, pair_rows="fp32")
    assert torch.equal(Ed, E0) and torch.equal(Fd, F0)  # the default is the keyword's "fp32"
    Er, Fr = ET.energy_and_forces(sd, hp, z, pos, batch, pair_rows="bf16")
    assert 1e-5 < rel(Fr, F0) < 2.0 ** -6  # the mode does round, by about a bf16 ulp


def test_periodic_box_and_fixture_with_identity_rounding(golden_dir):
    g = torch.load(os.path.join(golden_dir, "et_tiny_ref.pt"))
    sd, hp = B.f64(g["state_dict"]), ET.hparams_from_args(g["args"])
    box = torch.tensor([[11.0, 0.0, 0.0], [0.4, 11.5, 0.0], [0.3, -0.6, 10.6]], dtype=torch.float64)
    for bx in (None, box):
        E0, F0 = ET.energy_and_forces(sd, hp, g["z"], g["pos"].double(), g["batch"], box=bx)
        E1, F1 = ET.energy_and_forces(sd, hp, g["z"], g["pos"].double(), g["batch"], box=bx, pair_rows=lambda x: x)
        assert rel(E1, E0) < 1e-12 and rel(F1, F0) < 1e-12


def test_rounded_rows_are_bf16_values_and_bf16_tangents():
    sd, hp, _, _, _ = _tiny("both")
    R = "representation_model."
    means, betas = sd[R + "distance_expansion.means"], sd[R + "distance_expansion.betas"]
    d = torch.cat([torch.zeros(1, dtype=torch.float64), torch.linspace(0.05, 4.999, 97, dtype=torch.float64)]).requires_grad_(True)
    key = R + "attention_layers.1.dv_proj"
    rows = ET.rounded_filter_rows(sd, key, d, means, betas, 0.0, 5.0)
    plain = torch.nn.functional.silu(ET.lin(ET.expnorm_rbf(d, means, betas, 0.0, 5.0), sd, key))
    assert torch.equal(rows.detach(), ET.bf16_rne(plain.detach())) and not torch.equal(rows.detach(), plain.detach())
    assert torch.equal(rows.detach().float().bfloat16().double(), rows.detach())  # representable
    for c in (0, 17, 95):  # the derivative is the rounded tangent, element by element
        (t,) = torch.autograd.grad(rows[:, c].sum(), d, retain_graph=True)
        (t0,) = torch.autograd.grad(plain[:, c].sum(), d, retain_graph=True)
        assert torch.equal(t, ET.bf16_rne(t0)) and not torch.equal(t, t0)
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.0 - 2.0 ** -8], dtype=torch.float64)
    assert ET.bf16_rne(x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0]  # ties to even, not truncation


@pytest.mark.parametrize("di,widths", [("none", []), ("keys", [1]), ("values", [3]), ("both", [1, 3])])
def test_only_the_projections_that_exist_are_rounded(di, widths):
    sd, hp, z, pos, batch = _tiny(di)
    seen = []

    def spy(x):
        seen.append(x.shape[1])
        return ET.bf16_rne(x)

    E1, F1 = ET.energy_and_forces(sd, hp, z, pos, batch, pair_rows=spy)
    F = hp["hidden_channels"]
    assert seen == [w * F for w in widths for _ in range(2)] * hp["num_layers"]  # value and tangent of each, per layer
    E0, F0 = ET.energy_and_forces(sd, hp, z, pos, batch)
    Eb, Fb = ET.energy_and_forces(sd, hp, z, pos, batch, pair_rows="bf16")
    assert torch.equal(Eb, E1) and torch.equal(Fb, F1)
    if di == "none":  # no stored rows: the neighbour embedding's filter stays unrounded
        assert torch.equal(E1, E0) and torch.equal(F1, F0)
    else:
        assert not torch.equal(F1, F0)


# ---- noise floor and power of BF16_ORACLE_REL ---------------------------------------------------------------------------------
def _record():
    with open(os.path.join(ROOT, "profiles", "et_bf16_oracle_floor.json")) as fh:
        return json.load(fh)


def test_the_gpu_bound_is_the_recorded_one_and_covers_every_tile_case():
    from tests import test_gpu_et as G

    rec = _record()
    assert G.BF16_ORACLE_REL == rec["bound"]
    want = [c for c in G.TILE_CASES if c[3] != "none"]
    assert [tuple(c) for c in B.TILE_CASES] == want and sorted(rec["cases"]) == sorted(B.case_name(c) for c in want)
    for name, r in rec["cases"].items():
        assert 4 * r["floor"] <= rec["bound"] <= 0.5 * r["effect"], name


@pytest.mark.parametrize("case", B.TILE_CASES, ids=B.case_name)
def test_bound_clears_the_noise_floor_and_catches_unrounded_rows(case):
    """recomputed from the oracle: a correct engine (rows off by fp32 rounding and interpolation) stays 4 x below the bound,
    one that does not round its rows lands 2 x above it"""
    rec = _record()
    r = B.measure(case)
    print(B.case_name(case), r, "bound", rec["bound"])
    assert rec["bound"] >= 4 * r["floor"], r
    assert rec["bound"] <= 0.5 * r["effect"], r
    was = rec["cases"][B.case_name(case)]
    assert abs(r["effect"] - was["effect"]) < 0.02 * was["effect"] and abs(r["floor"] - was["floor"]) < 0.25 * was["floor"]


def test_value_only_rounding_is_caught():
    """the tangent rows left unrounded (the other half of `forgot to round`): still more than the bound away"""
    case = B.TILE_CASES[0]
    args, sd = B.tile_case_model(case)
    sd, hp = B.f64(sd), ET.hparams_from_args(args)
    z, pos, batch = W.synthetic_batch(n_mol=1, n_atoms=case[1], first_seed=300)
    calls = [0]

    def values_only(x):  # rounded_filter_rows rounds the value first, then the tangent
        calls[0] += 1
        return ET.bf16_rne(x) if calls[0] % 2 else x

    _, Fr = ET.energy_and_forces(sd, hp, z, pos.double(), batch, pair_rows="bf16")
    _, Fv = ET.energy_and_forces(sd, hp, z, pos.double(), batch, pair_rows=values_only)
    assert rel(Fv, Fr) > _record()["bound"]


# ---- bindings -------------------------------------------------------------------------------------------------------------------
def test_pair_storage_spellings():
    from torchmdnet_amd.models.model import PAIR_STORAGE, create_model

    assert PAIR_STORAGE == {"fp32": 0.0, "bf16": 1.0, "bf16-values": 2.0}
    for s in PAIR_STORAGE:
        m = create_model(dict(W.ET_TINY_ARGS, pair_storage=s))
        assert m.pair_storage == s
    m.pair_storage = "fp32"
    assert m.pair_storage == "fp32"
    with pytest.raises(ValueError):
        m.pair_storage = "fp16"
    with pytest.raises(ValueError):
        create_model(dict(W.ET_TINY_ARGS, pair_storage="bf16_values"))
    assert create_model(dict(W.ET_TINY_ARGS)).pair_storage == "fp32"
    tn2 = dict(W.TINY_ARGS, model="tensornet2", output_model="ScalarPlusWeightedCoulomb", q_dim=8, q_weights=[1.0, 0.5, 2.0])
    for args in (W.TINY_ARGS, tn2):
        assert create_model(dict(args)).pair_storage == "fp32"
        for s in ("bf16", "bf16-values"):
            with pytest.raises(NotImplementedError):
                create_model(dict(args, pair_storage=s))


def test_header_documents_the_values_mode_and_stays_additive():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)  # no new export, no changed argument list
    doc = re.search(r"/\*((?:(?!\*/).)*?\"pair_rows_bf16\".*?)\*/\s*int tmdnet_set_option", txt, flags=re.S).group(1)
    assert re.search(r"\b2: a developer and test mode", doc) and "dkv<l>" in doc and "tkv<l>" in doc
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert len(re.search(r"\bint\s+tmdnet_set_option\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")) == 3
    assert len(re.search(r"\bint\s+tmdnet_debug_tensor\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")) == 5
    for doc_file in ("INTEGRATION.md", "DESIGN.md"):
        assert "bf16-values" in open(os.path.join(ROOT, doc_file)).read(), doc_file
