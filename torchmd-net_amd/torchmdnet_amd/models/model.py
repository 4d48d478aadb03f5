# Host glue mirroring torchmd-net's torchmdnet/models/model.py (Copyright Universitat Pompeu Fabra 2020-2023,
# https://www.compscience.org, MIT License): `load_ensemble`, `create_prior_models`, `Ensemble` and the checkpoint
# key-rename / remix rules of `load_model` restate the reference's logic (model.py:167-205, 261-372, 377-448, 634-680)
# because they ARE the checkpoint / argument contract; everything numerical is this repository's own HIP code.
"""Model assembly with the reference's public surface (torchmdnet/models/model.py):
``create_model(args, prior_model=None, mean=None, std=None)``, ``load_model(filepath, args=None, device="cpu",
return_std=False, **kwargs)``, ``load_ensemble``, ``create_prior_models`` and the ``TorchMD_Net`` /
``Ensemble`` modules whose ``forward(z, pos, batch, box, q, s, extra_args, num_systems) -> (y, neg_dy)``
keeps the reference's conventions (model.py:530-631).

Everything numerical happens behind the C ABI of libtmdnet_amd.so (include/tmdnet_amd.h): this file
only owns parameters (state-dict compatible with the reference), marshals
pointers, and maps status codes to the reference's exceptions.  There is no CPU path.
"""
import copy
import ctypes as C
import os
import re
import tempfile
import warnings
import zipfile
from glob import glob
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor, nn

from torchmdnet_amd import _C, captured, ops, priors
from torchmdnet_amd.models import output_modules
from torchmdnet_amd.models.utils import _ptr, _require_cuda, _stream_ptr, dtype_mapping


# --------------------------------------------------------------------------------------------------
def create_model(args, prior_model=None, mean=None, std=None):
    """Same argument dict as the reference (model.py:21-164); see ``_create_model`` for what the HIP path supports.  One
    key beyond the reference's: ``pair_storage`` = "fp32" (default) | "bf16" - Equivariant Transformer only: the per-pair
    distance-filter rows are STORED as bf16 between the kernels (the sweeps that stream them read half the bytes); all
    arithmetic stays fp32.  That is the "bf16" of BASELINE configs[3]; the reference has no bf16 mode to compare with
    (models/utils.py:715), so its accuracy is stated against the fp32 oracle (tests/test_gpu_et.py).  A third spelling,
    "bf16-values", is a developer and test mode: the rows are rounded exactly as "bf16" rounds them and stored as fp32, so the
    fp32-row kernels run on the values the bf16-row kernels read (no bandwidth gain; tests/test_gpu_et.py compares the two)."""
    model = _create_model(args, prior_model=prior_model, mean=mean, std=std)
    model.pair_storage = str(args.get("pair_storage", "fp32"))
    return model


PAIR_STORAGE = {"fp32": 0.0, "bf16": 1.0, "bf16-values": 2.0}  # spelling -> engine option "pair_rows_bf16"


# property heads (csrc/tn_heads.hip): head class -> engine head kind (tmdnet_set_output_head)
_PROPERTY_HEADS = {"DipoleMoment": _C.HEAD_DIPOLE_MOMENT, "ElectronicSpatialExtent": _C.HEAD_SPATIAL_EXTENT,
                   "EquivariantDipoleMoment": _C.HEAD_DIPOLE_MOMENT, "EquivariantElectronicSpatialExtent": _C.HEAD_SPATIAL_EXTENT,
                   "EquivariantVectorOutput": _C.HEAD_VECTOR}
_PROPERTY_ARGS = ("DipoleMoment", "ElectronicSpatialExtent", "VectorOutput")  # the `output_model` values that name them


def _create_model(args, prior_model=None, mean=None, std=None):
    """Supported on the HIP path: model in {"tensornet", "tensornet2", "equivariant-transformer"}, precision 32,
    prior_model any of Atomref, ZBL, D2 (one of each pair prior)."""
    dtype = dtype_mapping[args["precision"]]
    if "box_vecs" not in args:
        args["box_vecs"] = None
    if "static_shapes" not in args:
        args["static_shapes"] = False
    if "vector_cutoff" not in args:
        args["vector_cutoff"] = False
    if dtype != torch.float32:
        raise NotImplementedError("torchmdnet_amd computes in fp32 (BASELINE north_star); precision="
                                  f"{args['precision']} has no HIP path")
    shared_args = dict(
        hidden_channels=args["embedding_dimension"],
        num_layers=args["num_layers"],
        num_rbf=args["num_rbf"],
        rbf_type=args["rbf_type"],
        trainable_rbf=args["trainable_rbf"],
        activation=args["activation"],
        cutoff_lower=float(args["cutoff_lower"]),
        cutoff_upper=float(args["cutoff_upper"]),
        max_z=args["max_z"],
        max_num_neighbors=args["max_num_neighbors"],
        box_vecs=(torch.tensor(args["box_vecs"], dtype=dtype) if args["box_vecs"] is not None else None),
        dtype=dtype,
    )
    is_equivariant = False
    if args["model"] == "tensornet":
        from torchmdnet_amd.models.tensornet import TensorNet

        representation_model = TensorNet(
            equivariance_invariance_group=args["equivariance_invariance_group"],
            static_shapes=args["static_shapes"],
            **shared_args,
        )
    elif args["model"] == "equivariant-transformer":
        from torchmdnet_amd.models.torchmd_et import TorchMD_ET

        is_equivariant = True
        representation_model = TorchMD_ET(
            attn_activation=args["attn_activation"],
            num_heads=args["num_heads"],
            distance_influence=args["distance_influence"],
            neighbor_embedding=args["neighbor_embedding"],
            vector_cutoff=args["vector_cutoff"],
            static_shapes=args["static_shapes"],
            **shared_args,
        )
    elif args["model"] == "tensornet2":
        from torchmdnet_amd.models.tensornet2 import TensorNet2

        representation_model = TensorNet2(
            equivariance_invariance_group=args["equivariance_invariance_group"],
            static_shapes=args["static_shapes"],
            q_dim=args.get("q_dim", 0),
            output_charges=True if "Coul" in args["output_model"] else False,
            **shared_args,
        )
    elif args["model"] in ("graph-network", "transformer"):
        raise NotImplementedError(f'architecture {args["model"]} has no MI355X-native path in this build (SURVEY.md 8(f))')
    else:
        raise ValueError(f'Unknown architecture: {args["model"]}')

    if args.get("atom_filter", -1) > -1:
        if args["derivative"]:
            raise ValueError("Derivative and atom filter can't be used together")
        raise NotImplementedError("AtomFilter wrapper is out of scope of the energy+force path")

    if args["prior_model"] and prior_model is None:
        prior_model = create_prior_models(args)

    if args["output_model"] == "ScalarPlusWeightedCoulomb":
        if args["model"] != "tensornet2":
            raise NotImplementedError("ScalarPlusWeightedCoulomb needs the charge channels of TensorNet2")
        output_model = output_modules.ScalarPlusWeightedCoulomb(
            args["embedding_dimension"], activation=args["activation"], reduce_op=args["reduce_op"], dtype=dtype,
            static_shapes=args.get("static_shapes", False), num_hidden_layers=args.get("output_mlp_num_layers", 0),
            num_layers=args["num_layers"], q_dim=args.get("q_dim", 0), q_weights=args.get("q_weights", []),
            coulomb_cutoff=args.get("coulomb_cutoff", None), coulomb_max_num_neighbors=args.get("coulomb_max_num_neighbors", None),
            coulomb_neighbor_strategy=args.get("coulomb_neighbor_strategy", "brute"))
        return TorchMD_Net(representation_model, output_model, prior_model=prior_model, mean=mean, std=std,
                           derivative=args["derivative"], dtype=dtype)
    if args["model"] == "tensornet2":
        raise NotImplementedError("TensorNet2 has a HIP path with output_model: ScalarPlusWeightedCoulomb only")
    if args["output_model"] in _PROPERTY_ARGS:
        # reference model.py:134: the Equivariant Transformer takes the "Equivariant" variant of every head
        name = ("Equivariant" if is_equivariant else "") + args["output_model"]
        if name not in _PROPERTY_HEADS:
            raise NotImplementedError(f"output_model {name} has no HIP path (property heads: {', '.join(_PROPERTY_HEADS)})")
        output_model = getattr(output_modules, name)(
            args["embedding_dimension"], activation=args["activation"], reduce_op=args["reduce_op"], dtype=dtype,
            static_shapes=args.get("static_shapes", False), num_hidden_layers=args.get("output_mlp_num_layers", 0), num_layers=0)
        return TorchMD_Net(representation_model, output_model, prior_model=prior_model, mean=mean, std=std,
                           derivative=args["derivative"], dtype=dtype)
    if args["output_model"] not in ("Scalar", "EquivariantScalar"):
        raise NotImplementedError(f'output_model {args["output_model"]} has no HIP path (Scalar, ScalarPlusWeightedCoulomb)')
    if is_equivariant:  # reference model.py:134-135: "Scalar" on an equivariant model is EquivariantScalar
        output_model = output_modules.EquivariantScalar(
            args["embedding_dimension"], activation=args["activation"], reduce_op=args["reduce_op"], dtype=dtype,
            static_shapes=args.get("static_shapes", False), num_hidden_layers=args.get("output_mlp_num_layers", 0))
        return TorchMD_Net(representation_model, output_model, prior_model=prior_model, mean=mean, std=std,
                           derivative=args["derivative"], dtype=dtype)
    if args["output_model"] != "Scalar":
        raise NotImplementedError("EquivariantScalar needs an equivariant representation model")
    output_model = output_modules.Scalar(
        args["embedding_dimension"],
        activation=args["activation"],
        reduce_op=args["reduce_op"],
        dtype=dtype,
        static_shapes=args.get("static_shapes", False),
        num_hidden_layers=args.get("output_mlp_num_layers", 0),
        num_layers=0,
    )
    return TorchMD_Net(representation_model, output_model, prior_model=prior_model, mean=mean, std=std,
                       derivative=args["derivative"], dtype=dtype)


def load_ensemble(filepath, args=None, device="cpu", return_std=False, **kwargs):
    """List of checkpoints or a zip of ``*.ckpt`` files -> Ensemble (reference model.py:167-205)."""
    if isinstance(filepath, (list, tuple)):
        assert all(isinstance(f, str) for f in filepath), "Invalid filepath list."
        model_list = [load_model(f, args=args, device=device, **kwargs) for f in filepath]
    elif filepath.endswith(".zip"):
        with tempfile.TemporaryDirectory() as tmpdir:
            with zipfile.ZipFile(filepath, "r") as zf:
                zf.extractall(tmpdir)
            ckpt_list = glob(os.path.join(tmpdir, "*.ckpt"))
            assert len(ckpt_list) > 0, "No checkpoint files found in zip file."
            model_list = [load_model(f, args=args, device=device, **kwargs) for f in ckpt_list]
    else:
        raise ValueError("Invalid filepath. Must be a list of paths or a path to a zip file.")
    return Ensemble(model_list, return_std=return_std)


def _remix_rows(weight, bias):
    """Old checkpoints stored per-atom tensors as [N,F,3,3]; the gate/edge-weight linears then emit
    F*3 interleaved rows.  Reorder to the current 3*F blocks (reference model.py:296-331)."""
    a, b = weight.shape
    weight = weight.view(a // 3, 3, b).transpose(0, 1).reshape(a, b)
    bias = bias.view(a // 3, 3).transpose(0, 1).reshape(a)
    return weight.contiguous(), bias.contiguous()


def load_model(filepath, args=None, device="cpu", return_std=False, **kwargs):
    """Consume a Lightning checkpoint written by the reference (model.py:208-374): hyper_parameters
    (overridable through kwargs), ``model.`` key prefix, legacy key renames, missing ``distance.box``
    buffer, old-layout remix (auto-detected through ``check_errors`` or forced with
    ``compatibility_load``), Atomref enable toggle for ``remove_ref_energy=False``."""
    if isinstance(filepath, (list, tuple)) or filepath.endswith(".zip"):
        return load_ensemble(filepath, args=args, device=device, return_std=return_std, **kwargs)
    assert isinstance(filepath, str)
    ckpt = torch.load(filepath, map_location="cpu", weights_only=False)
    if args is None:
        args = ckpt["hyper_parameters"]
    delta_learning = args["remove_ref_energy"] if "remove_ref_energy" in args else False
    for key, value in kwargs.items():
        if key not in args:
            warnings.warn(f"Unknown hyperparameter: {key}={value}")
        args[key] = value
    if args["model"] in ("tensornetv2_alt", "tensornet-nqe"):
        args["model"] = "tensornet2"

    model = create_model(args)
    if delta_learning and "remove_ref_energy" in kwargs and not kwargs["remove_ref_energy"]:
        assert model.prior_model is not None and len(model.prior_model) > 0, (
            "Atomref prior must be added during training (with enable=False) for total energy prediction.")
        assert isinstance(model.prior_model[-1], priors.Atomref), "I expected the last prior to be Atomref."
        model.prior_model[-1].enable = True

    state_dict = {re.sub(r"^model\.", "", k): v for k, v in ckpt["state_dict"].items()}
    renames = [
        (r"output_model.output_network.(\d+).update_net.(\d+).", r"output_model.output_network.\1.update_net.layers.\2."),
        (r"output_model.output_network.([02]).(weight|bias)", r"output_model.output_network.layers.\1.\2"),
    ]
    for pat, rep in renames:
        state_dict = {re.sub(pat, rep, k): v for k, v in state_dict.items()}
    if "representation_model.distance.box" not in state_dict:
        state_dict["representation_model.distance.box"] = torch.zeros((3, 3), device="cpu")

    if ("coulomb_cutoff" in args and args["coulomb_cutoff"] is not None and "output_model.distance.box" not in state_dict
            and hasattr(model.output_model, "distance")):  # reference model.py:283-291
        state_dict["output_model.distance.box"] = torch.zeros((3, 3), device="cpu")

    is_old = "check_errors" in ckpt.get("hyper_parameters", {})
    if kwargs.get("compatibility_load", is_old):
        if is_old and "compatibility_load" not in kwargs:
            warnings.warn("Old-format checkpoint detected ('check_errors' found in hyper_parameters). Automatically "
                          "applying compatibility_load to remap linear-layer weights. Pass compatibility_load=False "
                          "to suppress this.")
        # only the TensorNet families carry these layers (reference model.py:333-372): an old Equivariant Transformer
        # checkpoint also has 'check_errors' in its hyper-parameters and must load untouched
        keys = []
        if args["model"] in ("tensornet", "tensornet2"):
            keys.append("representation_model.tensor_embedding.linears_scalar.1")
        if args["model"] == "tensornet":
            keys += [f"representation_model.layers.{l}.linears_scalar.2" for l in range(args["num_layers"])]
        for k in keys:
            state_dict[k + ".weight"], state_dict[k + ".bias"] = _remix_rows(state_dict[k + ".weight"], state_dict[k + ".bias"])

    model.load_state_dict(state_dict)
    return model.to(device)


def create_prior_models(args, dataset=None):
    """Parse ``prior_model`` / ``prior_args`` exactly like the reference (model.py:377-448); only priors
    that exist in torchmdnet_amd.priors can be instantiated (Atomref, ZBL, D2)."""
    prior_models = []
    if args["prior_model"]:
        prior_model = args["prior_model"]
        names, pargs = [], []
        if not isinstance(prior_model, list):
            prior_model = [prior_model]
        for prior in prior_model:
            if isinstance(prior, dict):
                for key, value in prior.items():
                    names.append(key)
                    pargs.append({} if value is None else value)
            else:
                names.append(prior)
                pargs.append({})
        if "prior_args" in args and args["prior_args"] is not None:
            pargs = args["prior_args"]
            if not isinstance(pargs, list):
                pargs = [pargs]
        for name, arg in zip(names, pargs):
            if name == "Coulomb":
                raise NotImplementedError("prior model Coulomb has no MI355X-native path: it needs per-atom partial_charges through "
                                          "extra_args, which the registered operator tmdnet::energy_forces does not carry "
                                          f"(available: {priors.__all__})")
            if name not in priors.__all__:
                raise NotImplementedError(f"prior model {name} has no MI355X-native path (available: {priors.__all__})")
            prior_models.append(getattr(priors, name)(dataset=dataset, **arg))
    return prior_models


# --------------------------------------------------------------------------------------------------
class _EngineState:
    """Per-module handle of the HIP library + caller-owned workspaces.  Never copied or pickled."""

    def __init__(self):
        self.handle = None
        self.fingerprint = None
        self.tensors = None
        self.graph_ws = None
        self.fwd_ws = None
        self.virial_ws = None  # scratch of tmdnet_energy_forces_virial
        self.counts = None
        self.op_key = None   # key of the owning module in torchmdnet_amd.ops' registry (custom-op calls carry it)
        self.generation = 0  # bumped whenever the handle or a workspace is re-created: captured graphs of older generations are stale
        self.uploaded_fp = None   # fingerprint of the last FULL upload / device update (tmdnet_update_params_device)
        self.slot_keys = None     # state-dict key of every fingerprinted tensor
        self.device_updates = 0   # parameter updates that stayed on the GPU

    def release(self):
        if self.handle is not None:
            _C.lib().tmdnet_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def __deepcopy__(self, memo):
        return _EngineState()

    def __getstate__(self):
        return {}

    def __setstate__(self, state):
        self.__init__()


class _EnergyParamGrad(torch.autograd.Function):
    """E(theta) with d/d theta from the engine's parameter-gradient pass: forward half here (activations stay in the model's
    workspaces), reverse half in backward - or the whole pass again if another call used the workspaces in between."""

    @staticmethod
    def forward(ctx, model, z, pos, batch, box, q, n_mol, *params):
        if model._is_et() or model._is_tn2():  # one-call form: energies from the inference schedule here, the whole pass in backward
            energy, _ = model.energy_and_forces(z, pos, batch, box, q, n_mol, want_forces=False)
            _, token = model._train_forward(z, pos, batch, box, q, n_mol, keep=False)
        else:
            energy, token = model._train_forward(z, pos, batch, box, q, n_mol, keep=True)
        ctx.model, ctx.token, ctx.params = model, token, params
        return energy

    @staticmethod
    def backward(ctx, g_energy):
        grads = ctx.model._train_backward(ctx.token, g_energy)
        out = []
        for p in ctx.params:
            g = grads.get(p)
            out.append(None if g is None or not p.requires_grad else g.to(device=p.device, dtype=p.dtype).reshape(p.shape))
        return (None,) * 7 + tuple(out)


class _direct_radial_functions:
    """Scope in which the engine evaluates the radial functions directly (no radial tables): the inference-schedule calls INSIDE a
    training step - the weights change every step, re-tabulating would cost ~16 ms each.  The embedding in the radial basis stays on
    (its weight images are rebuilt on the device with every parameter update).  The previous values are restored on exit, so later
    validation / MD calls on the same module keep the benchmarked schedule."""

    NAMES = ("edge_table_min_pairs",)

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        m, L = self.model, _C.lib()
        st = m._sync_engine()
        self.saved_options = dict(getattr(st, "options", {}))
        self.saved = {}
        for n in self.NAMES:
            v = C.c_double()
            L.tmdnet_get_info(st.handle, n.encode(), C.byref(v))
            self.saved[n] = v.value
            L.tmdnet_set_option(st.handle, n.encode(), 1e15)
        st.options = dict(self.saved_options, **{n: 1e15 for n in self.NAMES})  # a re-upload inside the scope keeps them
        return self

    def __exit__(self, *exc):
        st = self.model._engine
        st.options = self.saved_options
        if st.handle is not None:
            for n, v in self.saved.items():
                _C.lib().tmdnet_set_option(st.handle, n.encode(), v)
        return False


class _EnergyForceParamGrad(torch.autograd.Function):
    """(E, F)(theta): d E / d theta exact (parameter-gradient pass); d (g_F . F) / d theta = - d/d theta of the directional
    derivative s = v . d(sum_m E_m)/d pos along v = g_F.  Every architecture (TensorNet + Scalar, the Equivariant Transformer,
    TensorNet2 + its Coulomb head) takes the ANALYTIC pass: the engine's second-order pass tmdnet_force_param_grads /
    tmdnet_loss_param_grads, the forward-mode tangent along v of its forward + reverse program (csrc/tn_hvp_api.hip), which is what
    the reference's second autograd pass computes (create_graph=True, model.py:618-628 + the *_bwd_bwd kernels); compared directly
    with the unmodified reference's double backward at 1e-4 on five fixtures (tests/test_gpu_hvp.py; measured 3e-6 .. 5e-6).
    A loss of energies AND forces is ONE seeded pass (`one_pass_training`); `H v` lands in pos.grad.
    `model.force_gradient_order = 2 / 4` keeps a central difference of the exact parameter gradient at pos +- h v / max|v|
    (`model.force_gradient_step` = h in Angstrom; 3e-4 / 1e-4 measured) as a cross-check for tests - slower than the analytic pass on
    all three architectures (profiles/r05_second_order_time.json) and not a parity path."""

    @staticmethod
    def forward(ctx, model, z, pos, batch, box, q, n_mol, *params):
        with _direct_radial_functions(model):
            energy, forces = model.energy_and_forces(z, pos, batch, box, q, n_mol, want_forces=True)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None in backward: no `.any()` read-back needed
        ctx.model, ctx.n_mol, ctx.params = model, n_mol, params
        ctx.save_for_backward(z, pos, batch, forces, *(t for t in (box, q) if t is not None))
        ctx.has = (box is not None, q is not None)
        return energy, forces

    @staticmethod
    def backward(ctx, g_energy, g_forces):
        z, pos, batch, forces, *rest = ctx.saved_tensors
        box = rest.pop(0) if ctx.has[0] else None
        q = rest.pop(0) if ctx.has[1] else None
        model, n_mol = ctx.model, ctx.n_mol
        total = {}

        def add(grads, w):
            for p, g in grads.items():
                gw = g if w == 1.0 else g * w
                total[p] = gw if p not in total else total[p] + gw

        if g_energy is None and g_forces is None:
            return (None,) * (7 + len(ctx.params))
        has_e, has_f = g_energy is not None, g_forces is not None  # (an all-zero gradient just costs its pass: no host read-back here)
        order = getattr(model, "force_gradient_order", None)
        order = int(order or 0)  # None / 0: the analytic pass (every architecture); 2 / 4: the difference-quotient cross-check
        analytic = order == 0
        # one pass for both terms: the analytic second-order pass with the energy seed ge = d loss / d E (tmdnet_loss_param_grads)
        one_pass = has_e and has_f and analytic and getattr(model, "one_pass_training", True)
        if has_e and not one_pass:
            add(model.parameter_gradients_of(z, pos, batch, box, q, n_mol, g_energy)[1], 1.0)
        g_pos = None
        pos_hv = ctx.needs_input_grad[2] and getattr(model, "force_position_gradient", True)
        if pos_hv and has_f and any(p is not None for p in model._pair_priors()):
            # H v of the model alone would lack the ZBL / D2 term: the parameter gradients (which the priors do not enter) stay exact,
            # pos.grad keeps the energy term's part only - said once, as for the difference-quotient orders below
            pos_hv = False
            if not getattr(model, "_warned_prior_pos_grad", False):
                warnings.warn("torchmdnet_amd: with a ZBL / D2 prior, pos.grad of a loss that depends on the FORCES holds only the "
                              "energy term's part (-g_E F): the pair priors have no second-derivative pass", stacklevel=2)
                model._warned_prior_pos_grad = True
        if g_energy is not None and not (one_pass and pos_hv):
            g_pos = -g_energy.reshape(-1)[batch].unsqueeze(1) * forces  # first order in pos (as tmdnet::energy_forces' backward)
        if has_f:
            v = g_forces.detach().to(torch.float32)
            want_hv = pos_hv
            with_hv = analytic and want_hv
            if want_hv and not analytic and not getattr(model, "_warned_pos_grad", False):
                # pos always requires grad here (the reference's side effect, model.py:584-585), so this cannot tell a caller who
                # wants d loss / d pos from one who does not: say it once instead of silently returning a truncated gradient.
                # (force_position_gradient = False is the caller's own choice: no warning then.)
                warnings.warn("torchmdnet_amd: pos.grad of a loss that depends on the FORCES holds only the energy term's part "
                              "(-g_E F): the difference-quotient force gradient (force_gradient_order 2 / 4) carries a graph to "
                              "the parameters only; the second derivative in the positions comes with the analytic pass "
                              "(force_gradient_order = None / 0, the default)", stacklevel=2)
                model._warned_pos_grad = True
            if analytic:
                # analytic second-order pass: d (g_F . F) / d theta = - d/d theta [ g_F . d sum_m E_m / d pos ],
                # and in the positions - H g_F (H = Hessian of the summed energy)
                seed = g_energy.detach().reshape(-1) if one_pass else None  # then gth / hv are the gradients of s - sum_m ge_m E_m
                # scale = -1: d loss / d theta through the forces is MINUS the pass' result - applied once to its flat output
                # instead of one multiply per parameter
                if with_hv:
                    gth, hv = model.force_term_parameter_gradients(z, pos.detach(), batch, box, q, n_mol, v, want_hv=True, ge=seed, scale=-1.0)
                    g_pos = hv if g_pos is None else g_pos + hv
                else:
                    gth = model.force_term_parameter_gradients(z, pos.detach(), batch, box, q, n_mol, v, ge=seed, scale=-1.0)
                add(gth, 1.0)
            else:
                scale = v.abs().max()
                vh = v / scale
                h = getattr(model, "force_gradient_step", None)
                h = float(h) if h else (0.02 if order >= 4 else 0.005)  # measured optimum of each order (profiles/r03_notes.md)
                ones = torch.ones(n_mol, dtype=torch.float32, device=pos.device)
                p0 = pos.detach()
                G = lambda t: model.parameter_gradients_of(z, p0 + t * vh, batch, box, q, n_mol, ones)[1]
                if order >= 4:  # (-f(2h) + 8 f(h) - 8 f(-h) + f(-2h)) / 12h
                    for t, w in ((2 * h, -1.0), (h, 8.0), (-h, -8.0), (-2 * h, 1.0)):
                        add(G(t), -float(scale) * w / (12 * h))
                else:
                    add(G(h), -float(scale) / (2 * h))
                    add(G(-h), float(scale) / (2 * h))
        out = []
        for p in ctx.params:
            g = total.get(p)
            out.append(None if g is None or not p.requires_grad else g.to(device=p.device, dtype=p.dtype).reshape(p.shape))
        return (None, None, g_pos, None, None, None, None) + tuple(out)


class TorchMD_Net(nn.Module):
    """Representation + output head + priors (reference model.py:451-631), evaluated by one fused HIP schedule."""

    def __init__(self, representation_model, output_model, prior_model=None, mean=None, std=None, derivative=False,
                 dtype=torch.float32):
        super().__init__()
        self.representation_model = representation_model.to(dtype=dtype)
        self.output_model = output_model.to(dtype=dtype)
        if not output_model.allow_prior_model and prior_model is not None:
            prior_model = None
            warnings.warn("Prior model was given but the output model does not allow prior models. Dropping the prior model.")
        if isinstance(prior_model, priors.BasePrior):
            prior_model = [prior_model]
        if prior_model is not None:
            for p in prior_model:
                if not isinstance(p, (priors.Atomref, priors.ZBL, priors.D2)):
                    raise NotImplementedError(f"prior {type(p).__name__} has no MI355X-native path")
            for kind in (priors.ZBL, priors.D2):  # the pair pass evaluates one prior of each kind
                if sum(isinstance(p, kind) for p in prior_model) > 1:
                    raise NotImplementedError(f"several {kind.__name__} priors in one model have no MI355X-native path")
        self.prior_model = None if prior_model is None else nn.ModuleList(prior_model).to(dtype=dtype)
        self.derivative = derivative
        mean = torch.scalar_tensor(0) if mean is None else mean
        self.register_buffer("mean", mean.to(dtype=dtype))
        std = torch.scalar_tensor(1) if std is None else std
        self.register_buffer("std", std.to(dtype=dtype))
        self._engine = _EngineState()
        self._pair_storage = "fp32"  # "bf16": Equivariant Transformer pair rows in reduced-precision storage (create_model)
        self.static_check = True  # static_shapes mode: poll the overflow flag after every non-captured call
        self.cell_list_min_atoms = 1024  # single periodic systems at least this large use the O(N) cell list
        # True: the outputs carry an autograd graph to the PARAMETERS: loss(y, F).backward() fills .grad of every weight - d y / d theta
        # exactly from the engine's parameter-gradient pass, d F / d theta from its analytic second-order pass along d loss / d F
        # (force matching; one seeded pass for a loss of both).  The reference needs no switch (autograd records
        # everything); here the default call stays on the inference schedule (radial tables, no saved activations)
        self.parameter_gradients = False
        self.force_position_gradient = True  # analytic pass: also - H g_F into pos.grad (False: the energy term's part only, a little faster)
        self.force_gradient_step = None  # Angstrom: largest atom displacement of the finite-difference direction (None: 0.005 / 0.02)
        # None / 0: analytic second-order pass (all three architectures) ; 2 / 4: central difference, two / four extra passes (tests)
        self.force_gradient_order = None
        # loss(E, F).backward() with the analytic pass: True = ONE seeded second-order pass delivers the energy term's gradient too
        # (tmdnet_loss_param_grads); False = the first-order pass for the energy term plus the second-order pass for the forces
        self.one_pass_training = True
        self.reset_parameters()

    def reset_parameters(self):
        self.representation_model.reset_parameters()
        self.output_model.reset_parameters()
        if self.prior_model is not None:
            for prior in self.prior_model:
                prior.reset_parameters()

    # ---------------------------------------------------------------- engine plumbing
    def _hparams(self) -> _C.HParams:
        rm = self.representation_model
        hp = _C.HParams()
        hp.hidden_channels = rm.hidden_channels
        hp.num_layers = rm.num_layers
        hp.num_rbf = rm.num_rbf
        hp.max_z = rm.max_z
        hp.max_num_neighbors = rm.max_num_neighbors
        hp.group_o3 = 1 if rm.equivariance_invariance_group == "O(3)" else 0
        hp.head_hidden = self.output_model.output_network.layers[0].out_features
        hp.has_atomref = 1 if self._atomref_table() is not None else 0
        hp.cutoff_lower = float(rm.cutoff_lower)
        hp.cutoff_upper = float(rm.cutoff_upper)
        return hp

    def _head_kind(self) -> int:
        """Engine output head: scalar energies, or one of the property heads (tmdnet_set_output_head)."""
        return _PROPERTY_HEADS.get(type(self.output_model).__name__, _C.HEAD_SCALAR)

    def _is_et(self) -> bool:
        return type(self.representation_model).__name__ == "TorchMD_ET"

    def _is_tn2(self) -> bool:
        return type(self.representation_model).__name__ == "TensorNet2"

    def _tn2_hparams(self) -> _C.Tn2HParams:
        rm, om = self.representation_model, self.output_model
        hp = _C.Tn2HParams()
        hp.hidden_channels = rm.hidden_channels
        hp.num_layers = rm.num_layers
        hp.num_rbf = rm.num_rbf
        hp.max_z = rm.max_z
        hp.max_num_neighbors = rm.max_num_neighbors
        hp.group_o3 = 1 if rm.equivariance_invariance_group == "O(3)" else 0
        hp.head_hidden = om.output_network.layers[0].out_features
        hp.has_atomref = 1 if self._atomref_table() is not None else 0
        hp.q_dim = rm.q_dim
        hp.cutoff_lower = float(rm.cutoff_lower)
        hp.cutoff_upper = float(rm.cutoff_upper)
        hp.coulomb_cutoff = -1.0 if om.cutoff is None else float(om.cutoff)
        hp.coulomb_epsilon_solvent = float(om.epsilon_solvent)
        return hp

    def _et_hparams(self) -> _C.EtHParams:
        rm = self.representation_model
        hp = _C.EtHParams()
        hp.hidden_channels = rm.hidden_channels
        hp.num_layers = rm.num_layers
        hp.num_rbf = rm.num_rbf
        hp.max_z = rm.max_z
        hp.max_num_neighbors = rm.max_num_neighbors
        hp.num_heads = rm.num_heads
        hp.neighbor_embedding = 1 if rm.neighbor_embedding is not None else 0
        hp.vector_cutoff = 1 if rm.vector_cutoff else 0
        hp.distance_influence = {"none": 0, "keys": 1, "values": 2, "both": 3}[rm.distance_influence]
        hp.has_atomref = 1 if self._atomref_table() is not None else 0
        hp.cutoff_lower = float(rm.cutoff_lower)
        hp.cutoff_upper = float(rm.cutoff_upper)
        return hp

    def _atomref_table(self) -> Optional[Tensor]:
        if self.prior_model is None:
            return None
        tables = [p.atomref.weight.detach().reshape(-1) for p in self._atomref_priors() if p.enable]
        if not tables:
            return None
        max_z = self.representation_model.max_z
        out = torch.zeros(max_z, dtype=torch.float32)
        for t in tables:
            n = min(max_z, t.numel())
            out[:n] += t[:n].float().cpu()
        return out

    def _atomref_priors(self):
        return [p for p in (self.prior_model or ()) if isinstance(p, priors.Atomref)]

    def _pair_priors(self):
        """(ZBL or None, D2 or None): the priors that the pair pass behind the engine call evaluates (csrc/tn_prior.hip)."""
        zbl = d2 = None
        for p in (self.prior_model or ()):
            if isinstance(p, priors.ZBL):
                zbl = p
            elif isinstance(p, priors.D2):
                d2 = p
        return zbl, d2

    def _stage_pair_priors(self, st):
        """Upload the species tables and unit scales of the ZBL / D2 priors (``tmdnet_set_pair_priors``), or clear them."""
        import numpy as np

        L = _C.lib()
        zbl, d2 = self._pair_priors()
        st.pair_priors = zbl is not None or d2 is not None
        if not st.pair_priors:
            L.tmdnet_set_pair_priors(st.handle, None)
            return
        max_z = int(self.representation_model.max_z)
        pp = _C.PairPriors()
        pp.max_z = max_z
        keep = []  # the host tables, alive until the call has copied them
        host = lambda a: keep.append(np.ascontiguousarray(a, dtype=np.float32)) or keep[-1].ctypes.data
        if zbl is not None:
            pp.flags |= _C.PRIOR_ZBL
            pp.zbl_cutoff, pp.zbl_distance_scale, pp.zbl_energy_scale = float(zbl.cutoff_distance), zbl.distance_scale, zbl.energy_scale
            Z, Z23 = zbl.species_tables(max_z)
            pp.zbl_z, pp.zbl_z23 = host(Z), host(Z23)
        if d2 is not None:
            pp.flags |= _C.PRIOR_D2
            pp.d2_cutoff, pp.d2_distance_scale, pp.d2_energy_scale = float(d2.cutoff_distance), float(d2.distance_scale), float(d2.energy_scale)
            sq, rr = d2.species_tables(max_z)
            pp.d2_sqrt_c6, pp.d2_rr = host(sq), host(rr)
        if L.tmdnet_set_pair_priors(st.handle, C.byref(pp)) != _C.OK:
            raise RuntimeError(f"tmdnet_set_pair_priors: {L.tmdnet_last_error(st.handle).decode()}")

    def _refuse_pair_priors(self, what):
        """What the pair priors are not implemented for: raised before anything is set on the handle."""
        if any(p is not None for p in self._pair_priors()):
            raise NotImplementedError(f"the ZBL / D2 pair priors have no HIP path with {what}")

    def _check_pair_prior_inputs(self, z, batch, n_mol):
        """Host-side refusals of the pair pass that depend on the inputs: a D2 species without a table entry, and a molecule beyond
        the brute-force limit.  Read back once per ``z`` / ``batch`` tensor and version (an MD loop keeps them: no synchronisation
        per step), never during a capture."""
        key = (z.data_ptr(), z._version, tuple(z.shape), batch.data_ptr(), batch._version, n_mol)
        if getattr(self._engine, "prior_checked", None) == key or torch.cuda.is_current_stream_capturing():
            return
        d2 = self._pair_priors()[1]
        if d2 is not None:
            d2.check_species(z)
        if z.shape[0] > priors.MAX_MOLECULE_ATOMS:
            priors.check_molecule_size(int(torch.bincount(batch.reshape(-1).clamp(min=0)).max()))
        self._engine.prior_checked = key

    def _add_pair_priors(self, st, stream, n, n_mol, p32, z, batch, box, box_mode, energy, forces, virial):
        """The pair pass behind an engine call: ADDS the ZBL / D2 energies, forces and virial on the same stream
        (``tmdnet_pair_priors_add``: three launches, no read-back).  One zeroed workspace per (n, n_mol), as the pass wants it."""
        L = _C.lib()
        dev = p32.device
        nbytes = C.c_size_t(0)
        L.tmdnet_pair_priors_workspace_bytes(st.handle, n, n_mol, C.byref(nbytes))
        pool = getattr(st, "prior_ws", None)
        if pool is None:
            pool = st.prior_ws = {}
        ws = pool.get((n, n_mol))
        if ws is None or ws.device != dev or ws.numel() < nbytes.value:
            if len(pool) >= 16:  # bounded: a captured graph may hold the address of a workspace that goes, so it becomes stale
                pool.clear()
                st.generation += 1
            ws = pool[(n, n_mol)] = torch.zeros(max(int(nbytes.value), 256), dtype=torch.uint8, device=dev)
        rc = L.tmdnet_pair_priors_add(st.handle, stream, _ptr(ws), ws.numel(), n, n_mol, _ptr(p32), _ptr(z), _ptr(batch), _ptr(box),
                                      box_mode, None, _ptr(energy), _ptr(forces), _ptr(virial))
        if rc == _C.ERR_INVALID:
            raise NotImplementedError(f"tmdnet_pair_priors_add: {L.tmdnet_last_error(st.handle).decode()}")
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_pair_priors_add: {L.tmdnet_last_error(st.handle).decode()} (code {rc})")

    def debug_pair_priors(self, z, pos, batch, box=None, num_systems=None, want_virial=True):
        """Test entry (``tmdnet_debug_prior``): the pair pass alone into zeroed outputs -> (E [B], F [N,3], W [B,3,3] or None,
        e_atom [N] fp64), the per-atom energies e_i = 1/2 sum_j u_ij included."""
        _require_cuda(pos, "TorchMD_Net.debug_pair_priors")
        L = _C.lib()
        dev = pos.device
        with torch.cuda.device(dev):
            st = self._sync_engine()
            n = int(z.shape[0])
            n_mol = int(num_systems) if num_systems is not None else (int(batch.max().item()) + 1 if n else 0)
            p32 = pos.detach().to(torch.float32).contiguous()
            z, batch = z.contiguous(), batch.to(torch.long).contiguous()
            box_mode = 0
            if box is not None:
                box = box.detach().to(device=dev, dtype=torch.float32).contiguous()
                box_mode = 1 if box.dim() == 2 else 2
            nbytes = C.c_size_t(0)
            L.tmdnet_pair_priors_workspace_bytes(st.handle, n, n_mol, C.byref(nbytes))
            ws = torch.empty(max(int(nbytes.value), 256), dtype=torch.uint8, device=dev)
            energy = torch.empty(n_mol, dtype=torch.float32, device=dev)
            forces = torch.empty((n, 3), dtype=torch.float32, device=dev)
            virial = torch.empty((n_mol, 3, 3), dtype=torch.float32, device=dev) if want_virial else None
            e_atom = torch.empty(n, dtype=torch.float64, device=dev)
            rc = L.tmdnet_debug_prior(st.handle, _stream_ptr(dev), _ptr(ws), ws.numel(), n, n_mol, _ptr(p32), _ptr(z), _ptr(batch), _ptr(box),
                                      box_mode, _ptr(energy), _ptr(forces), _ptr(virial), _ptr(e_atom))
            if rc != _C.OK:
                raise RuntimeError(f"tmdnet_debug_prior: {L.tmdnet_last_error(st.handle).decode()} (code {rc})")
        return energy, forces, virial, e_atom

    def _apply(self, fn, recurse=True):
        # .to() / .cuda() / .float() replace buffers by new tensor objects: drop the cached tensor list of _fingerprint
        self._engine.tensors = None
        return super()._apply(fn, recurse)

    def _index_tensors(self):
        """(owning dict, key, tensor) of every parameter / persistent buffer and (dict, key, child) of every submodule."""
        slots, mods, sizes = [], [], []
        for mod in self.modules():
            for k, p in mod._parameters.items():
                if p is not None:
                    slots.append((mod._parameters, k, p))
            for k, b in mod._buffers.items():
                if b is not None and k not in mod._non_persistent_buffers_set:
                    slots.append((mod._buffers, k, b))
            for k, ch in mod._modules.items():
                mods.append((mod._modules, k, ch))
            sizes.extend(((mod._parameters, len(mod._parameters)), (mod._buffers, len(mod._buffers)), (mod._modules, len(mod._modules))))
        return slots, mods, sizes

    def _fingerprint(self):
        """Cheap change detector for the uploaded parameters: (version, address) of every tensor of the state dict.  Walking
        the module tree costs more than a small MD step, so the (dict, key, tensor) slots are cached and only re-checked for
        IDENTITY: a replaced Parameter / buffer object (``load_state_dict(assign=True)``, ``mod.weight = nn.Parameter(..)``,
        a swapped submodule, a parametrization) no longer matches its slot and the index is rebuilt."""
        st = self._engine
        idx = st.tensors
        if idx is not None:
            slots, mods, sizes = idx
            if not (all(d.get(k) is t for d, k, t in slots) and all(d.get(k) is c for d, k, c in mods)
                    and all(len(d) == n for d, n in sizes)):
                idx = None
                st.index_epoch = getattr(st, "index_epoch", 0) + 1
        if idx is None:
            idx = st.tensors = self._index_tensors()
        fp = [getattr(st, "index_epoch", 0)]
        fp.extend((t._version, t.data_ptr()) for _, _, t in idx[0])
        if self.prior_model is not None:
            # Atomref: its switch; ZBL / D2: every argument the engine's copy depends on (they are plain attributes, not tensors)
            fp.append(tuple(p.enable if isinstance(p, priors.Atomref) else p.engine_key() for p in self.prior_model))
        return tuple(fp)

    @property
    def pair_storage(self) -> str:
        """ "fp32" | "bf16" | "bf16-values" (see ``create_model``).  Assigning it takes effect from the next call on, also on a model
        whose engine is already uploaded; replays captured before keep the mode they were captured with."""
        d = self.__dict__  # (a module pickled before the attribute became a property carries it under its public name)
        return d.get("_pair_storage", d.get("pair_storage", "fp32"))

    @pair_storage.setter
    def pair_storage(self, storage):
        storage = str(storage)
        if storage not in PAIR_STORAGE:
            raise ValueError(f"pair_storage must be one of {', '.join(repr(k) for k in PAIR_STORAGE)}, got {storage!r}")
        if storage != "fp32" and not self._is_et():
            raise NotImplementedError(f"pair_storage={storage!r} applies to the Equivariant Transformer only")
        self._pair_storage = storage
        if self._engine.handle is not None:  # the uploaded parameters stay: only the option changes
            _C.lib().tmdnet_set_option(self._engine.handle, b"pair_rows_bf16", PAIR_STORAGE[storage])

    def _sync_engine(self):
        """(Re)create the library handle and upload the parameters when they changed."""
        st = self._engine
        fp = self._fingerprint()
        if st.handle is not None and st.fingerprint == fp:
            return st
        dev = next(self.parameters()).device
        if dev.type == "cuda" and torch.cuda.current_device() != dev.index:
            # allocations and the device-side update must land on the MODEL's GPU, not on whatever device is current (a model on a
            # non-current GPU of a single multi-GPU process)
            with torch.cuda.device(dev):
                return self._sync_engine()
        L = _C.lib()
        hp = self._et_hparams() if self._is_et() else (self._tn2_hparams() if self._is_tn2() else self._hparams())
        hp_key = (type(hp).__name__, bytes(hp), self._head_kind())
        st.generation += 1  # captured replays of the previous weights are stale either way
        if st.handle is None or getattr(st, "hp_key", None) != hp_key:
            st.release()
            handle = C.c_void_p()
            create = L.tmdnet_create_et if self._is_et() else (L.tmdnet_create_tn2 if self._is_tn2() else L.tmdnet_create)
            rc = create(C.byref(hp), C.byref(handle))
            if rc != _C.OK:
                raise RuntimeError(f"tmdnet_create failed with code {rc}")
            if self._head_kind() != _C.HEAD_SCALAR and L.tmdnet_set_output_head(handle, self._head_kind()) != _C.OK:
                msg = L.tmdnet_last_error(handle).decode()
                L.tmdnet_destroy(handle)
                raise NotImplementedError(msg)
            st.handle, st.hp_key = handle, hp_key
        # else: same architecture, new weights (training loop): the handle and its device buffers are kept, the parameters
        # are re-uploaded below (hipFree / hipMalloc per step would each be a device-wide synchronisation)
        handle = st.handle
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        if self._update_engine_on_device(st, sd, fp):
            return st
        table = self._atomref_table()
        if table is not None:
            sd["atomref"] = table
        n = L.tmdnet_num_params(handle)
        for i in range(n):
            numel = C.c_int64()
            name = L.tmdnet_param_name(handle, i, C.byref(numel)).decode()
            if name not in sd:
                raise RuntimeError(f"state dict lacks parameter {name}")
            t = sd[name].to(device="cpu", dtype=torch.float32).contiguous().reshape(-1)
            rc = L.tmdnet_set_param(handle, name.encode(), C.c_void_p(t.data_ptr()), t.numel())
            if rc != _C.OK:
                raise RuntimeError(L.tmdnet_last_error(handle).decode())
        rc = L.tmdnet_finalize_params(handle)
        if rc != _C.OK:
            raise RuntimeError(L.tmdnet_last_error(handle).decode())
        if self.pair_storage != "fp32":
            L.tmdnet_set_option(handle, b"pair_rows_bf16", PAIR_STORAGE[self.pair_storage])
        for name, value in getattr(st, "options", {}).items():
            L.tmdnet_set_option(handle, name.encode(), value)
        self._stage_pair_priors(st)
        st.fingerprint = fp
        # state for the device-side update of the next training step: the fingerprint this upload corresponds to and the
        # state-dict key of every fingerprinted tensor (None: not in the state dict)
        st.uploaded_fp = fp
        by_id = {id(v): k for k, v in self.state_dict(keep_vars=True).items()}
        st.slot_keys = [by_id.get(id(t)) for _, _, t in st.tensors[0]]
        return st

    def _update_engine_on_device(self, st, sd, fp):
        """Training loops: same handle, same tensors, new values on the GPU -> ``tmdnet_update_params_device`` rewrites the
        engine's parameter buffer from the optimizer's tensors with a gather kernel (no host round trip of the weights, no
        synchronisation).  Taken when the full upload happened once with the same tensor objects, every tensor is a
        contiguous fp32 CUDA tensor, and nothing the host reads (mean, std, the Atomref table) changed."""
        if getattr(st, "uploaded_fp", None) is None or self._is_et() or not getattr(self, "device_parameter_update", True):
            return False
        old = st.uploaded_fp
        if len(old) != len(fp) or old[0] != fp[0]:
            return False
        slots = st.tensors[0]
        names, ptrs = [], []
        keys = st.slot_keys
        if keys is None or len(keys) != len(slots):
            return False
        for (name, (_, _, t)), o, n in zip(zip(keys, slots), old[1:], fp[1:]):
            if o == n:
                continue
            if o[1] != n[1] or name in ("mean", "std") or name is None or name.startswith("prior_model"):
                return False  # storage moved, or a tensor the host reads: full upload
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                return False
            names.append(name.encode())
            ptrs.append(t.data_ptr())
        if self.prior_model is not None and old[len(slots) + 1:] != fp[len(slots) + 1:]:
            return False
        if not names:
            return False
        L = _C.lib()
        arr_n = (C.c_char_p * len(names))(*names)
        arr_p = (C.c_void_p * len(ptrs))(*ptrs)
        rc = L.tmdnet_update_params_device(st.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream), len(names), arr_n, arr_p)
        if rc != _C.OK:
            return False  # e.g. a parameter the engine does not know by that name: the full upload reports it
        st.fingerprint = fp
        st.uploaded_fp = fp
        st.device_updates += 1
        return True

    # ---------------------------------------------------------------- parameter gradients (energy-only training)
    def _grad_targets(self):
        """engine gradient entry -> parameter(s) it belongs to (reference state-dict layout)"""
        rm, on = self.representation_model, self.output_model.output_network
        te = rm.tensor_embedding
        m = {"Ue%d" % k: te.linears_tensor[k].weight for k in range(3)}
        m.update({"L1": te.linears_scalar[0].weight, "bL1": te.linears_scalar[0].bias, "L2": te.linears_scalar[1].weight,
                  "bL2": te.linears_scalar[1].bias, "ln0_w": te.init_norm.weight, "ln0_b": te.init_norm.bias,
                  "lnr_w": rm.out_norm.weight, "lnr_b": rm.out_norm.bias, "Lin": rm.linear.weight, "bLin": rm.linear.bias,
                  "O1": on.layers[0].weight, "bO1": on.layers[0].bias, "O2": on.layers[2].weight, "bO2": on.layers[2].bias})
        for l, layer in enumerate(rm.layers):
            for k in range(3):
                m["l%d.M%d" % (l, k)] = layer.linears_scalar[k].weight
                m["l%d.b%d" % (l, k)] = layer.linears_scalar[k].bias
                m["l%d.Va%d" % (l, k)] = layer.linears_tensor[k].weight
                m["l%d.Vb%d" % (l, k)] = layer.linears_tensor[3 + k].weight
        return m

    def parameter_gradients_of(self, z, pos, batch, box, q, n_mol, grad_energy):
        """d(sum_m grad_energy[m] E_m)/d theta for every weight of TensorNet + Scalar: (E [n_mol], {parameter: gradient}).
        One engine call (tmdnet_energy_param_grads): forward with every pre-activation kept, reverse pass with the weight
        gradients taken where an adjoint meets its input; the species tables' gradients are chained to emb / emb2 here."""
        energy, token = self._train_forward(z, pos, batch, box, q, n_mol, keep=False)
        return energy, self._train_backward(token, grad_energy)

    def force_term_parameter_gradients(self, z, pos, batch, box, q, n_mol, v, want_hv=False, ge=None, scale=1.0):
        """d s / d theta of  s = v . d(sum_m E_m)/d pos = - v . F  for every weight of TensorNet + Scalar, analytically
        (tmdnet_force_param_grads: the tangent, along v, of the engine's forward + reverse program - what the reference gets from
        its second autograd pass, model.py:618-628 with create_graph=True).  -> {parameter: gradient}; d loss / d theta through
        the forces is MINUS this with v = d loss / d F.  want_hv: -> ({parameter: gradient}, H v [N, 3]) with H v = d s / d pos, the
        Hessian of the summed energy applied to v (the position gradient of such a loss is - H v).
        ge [n_mol] = d loss / d E (one-pass training, tmdnet_loss_param_grads): the gradients of  S = s - sum_m ge_m E_m  instead, so
        that the whole gradient of loss(E, F) is minus the result (parameters) and minus H v' (positions); an Atomref prior's table,
        which the engine does not hold, is added here."""
        if want_hv:  # H v of the model alone would lack the priors' second derivative
            self._refuse_pair_priors("second derivatives with respect to the positions (want_hv=True, a force loss's pos.grad); "
                                     "set force_position_gradient = False, or take hessian(method='central')")
        if self._is_et():
            q = None  # TorchMD_ET.forward ignores q
        L = _C.lib()
        dev = pos.device
        with torch.cuda.device(dev):
            st = self._sync_engine()
            stream = _stream_ptr(dev)
            n = int(z.shape[0])
            p32 = pos.detach().to(torch.float32).contiguous()
            v32 =v.detach().to(device=dev, dtype=torch.float32).contiguous()
            assert v32.shape == p32.shape
            z = z.contiguous()
            batch = batch.to(torch.long).contiguous()
            box_mode = 0
            if box is not None:
                box = box.detach().to(device=dev, dtype=torch.float32).contiguous()
                box_mode = 1 if box.dim() == 2 else 2
            if q is not None:
                q = q.detach().to(device=dev, dtype=torch.float32).contiguous()
            L.tmdnet_set_cell_grid(st.handle, 0, 0, 0)  # brute force inside each molecule (atoms keep their order)
            nbytes = C.c_size_t(0)
            L.tmdnet_graph_workspace_bytes(st.handle, n, n_mol, C.byref(nbytes))
            st.graph_ws = self._grow(st.graph_ws, nbytes.value, dev)
            counts = (C.c_int64 * 8)()
            rc = self._build_graph_for_a_training_pass(st, stream, n, n_mol, p32, batch, z, box, box_mode, counts)
            self._raise_bad_indices(counts, L.tmdnet_last_error(st.handle).decode())
            if rc != _C.OK:
                raise RuntimeError(L.tmdnet_last_error(st.handle).decode())
            n_pairs = int(counts[0])
            hb = C.c_size_t(0)
            if L.tmdnet_force_param_workspace_bytes(st.handle, n, n_mol, n_pairs, C.byref(hb)) != _C.OK:
                raise RuntimeError(L.tmdnet_last_error(st.handle).decode())
            st.hvp_ws = self._grow(getattr(st, "hvp_ws", None), hb.value, dev)
            gfl = C.c_int64(0)
            L.tmdnet_train_workspace_bytes(st.handle, n, n_mol, n_pairs, None, None, C.byref(gfl))
            flat = torch.empty(gfl.value, dtype=torch.float32, device=dev)
            hv = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_hv else None
            ge32 = None if ge is None else ge.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            assert ge32 is None or ge32.numel() == n_mol
            rc = L.tmdnet_loss_param_grads(st.handle, stream, _ptr(st.graph_ws), _ptr(st.hvp_ws), st.hvp_ws.numel(), n, n_mol, n_pairs,
                                           _ptr(z), _ptr(batch), _ptr(q), _ptr(v32), _ptr(ge32), _ptr(flat), _ptr(hv))
            if rc != _C.OK:
                raise RuntimeError(f"tmdnet_loss_param_grads: {L.tmdnet_last_error(st.handle).decode()} (code {rc})")
            st.ws_epoch = getattr(st, "ws_epoch", 0) + 1  # the graph workspace was rebuilt: a kept forward half is stale
            if scale != 1.0:  # every map below is linear in the flat buffer
                flat.mul_(scale)
                if hv is not None:
                    hv.mul_(scale)
            ent = {}
            for i in range(L.tmdnet_param_grad_count(st.handle)):
                off, numel = C.c_int64(0), C.c_int64(0)
                name = L.tmdnet_param_grad_entry(st.handle, i, C.byref(off), C.byref(numel)).decode()
                ent[name] = flat[off.value: off.value + numel.value]
            grads = self._et_grads(ent) if self._is_et() else (self._tn2_grads(ent) if self._is_tn2() else self._tensornet_grads(ent))
            if ge32 is not None and self.prior_model is not None:  # d S / d atomref[z] = - sum of ge[molecule] over the atoms of species z
                for pr in self._atomref_priors():
                    if pr.enable:
                        w = pr.atomref.weight
                        grads[w] = (-scale) * torch.zeros(w.shape[0], dtype=torch.float32, device=dev).index_add_(0, z, ge32[batch]).view_as(w)
            return (grads, hv) if want_hv else grads

    def _build_graph_for_a_training_pass(self, st, stream, n, n_mol, p32, batch, z, box, box_mode, counts):
        """tmdnet_build_graph for the parameter-gradient passes.  They evaluate the radial functions directly, so their graph needs
        neither the species map of the radial-basis embedding nor its weight images - which a device-side parameter update leaves
        stale, and whose rebuild (`k_embed_rb_images` on the update's stream, tn_embed_rb.hip) would otherwise be paid by every
        training step: the embedding's atom threshold is out of reach for the duration of this one call."""
        L = _C.lib()
        v = C.c_double()
        L.tmdnet_get_info(st.handle, b"embed_rb_min_atoms", C.byref(v))
        L.tmdnet_set_option(st.handle, b"embed_rb_min_atoms", 1e15)
        try:
            return L.tmdnet_build_graph(st.handle, stream, _ptr(st.graph_ws), st.graph_ws.numel(), n, n_mol, _ptr(p32), _ptr(batch),
                                        _ptr(z), _ptr(box), box_mode, counts)
        finally:
            L.tmdnet_set_option(st.handle, b"embed_rb_min_atoms", v.value)

    def _train_forward(self, z, pos, batch, box, q, n_mol, keep=True):
        """Forward half of the parameter-gradient pass.  keep=True: the activations stay in the model's workspaces and the
        returned token lets `_train_backward` run the reverse half on them - unless another engine call used the workspaces
        in between (the token's epoch no longer matches), in which case the pass is repeated from the inputs."""
        if self._is_tn2():
            keep = False  # one-call form only
        if self._is_et():
            keep, q = False, None  # one-call form only; TorchMD_ET.forward ignores q
        L = _C.lib()
        dev = pos.device
        with torch.cuda.device(dev):
            st = self._sync_engine()
            stream = _stream_ptr(dev)
            n = int(z.shape[0])
            p32 = pos.detach().to(torch.float32).contiguous()
            z = z.contiguous()
            batch = batch.to(torch.long).contiguous()
            box_mode = 0
            if box is not None:
                box = box.detach().to(device=dev, dtype=torch.float32).contiguous()
                box_mode = 1 if box.dim() == 2 else 2
            if q is not None:
                q = q.detach().to(device=dev, dtype=torch.float32).contiguous()
            L.tmdnet_set_cell_grid(st.handle, 0, 0, 0)  # brute force inside each molecule (atoms keep their order)
            nbytes = C.c_size_t(0)
            L.tmdnet_graph_workspace_bytes(st.handle, n, n_mol, C.byref(nbytes))
            st.graph_ws = self._grow(st.graph_ws, nbytes.value, dev)
            counts = (C.c_int64 * 8)()
            rc = self._build_graph_for_a_training_pass(st, stream, n, n_mol, p32, batch, z, box, box_mode, counts)
            self._raise_bad_indices(counts, L.tmdnet_last_error(st.handle).decode())
            if rc != _C.OK:
                raise RuntimeError(L.tmdnet_last_error(st.handle).decode())
            n_pairs = int(counts[0])
            fwd_b, trn_b, gfl = C.c_size_t(0), C.c_size_t(0), C.c_int64(0)
            rc = L.tmdnet_train_workspace_bytes(st.handle, n, n_mol, n_pairs, C.byref(fwd_b), C.byref(trn_b), C.byref(gfl))
            if rc != _C.OK:
                raise RuntimeError(L.tmdnet_last_error(st.handle).decode())
            st.fwd_ws = self._grow(st.fwd_ws, fwd_b.value, dev)
            st.train_ws = self._grow(getattr(st, "train_ws", None), trn_b.value, dev)
            energy = torch.empty(n_mol, dtype=torch.float32, device=dev)
            token = dict(z=z, pos=p32, batch=batch, box=box, q=q, n=n, n_mol=n_mol, n_pairs=n_pairs, grad_floats=gfl.value, dev=dev,
                         handle=st.handle.value, epoch=None, energy=energy)
            if keep:
                rc = L.tmdnet_energy_param_grads(st.handle, stream, _ptr(st.graph_ws), _ptr(st.fwd_ws), st.fwd_ws.numel(),
                                                 _ptr(st.train_ws), st.train_ws.numel(), n, n_mol, n_pairs, _ptr(z), _ptr(batch), _ptr(q),
                                                 None, _ptr(energy), None)
                if rc != _C.OK:
                    raise RuntimeError(f"tmdnet_energy_param_grads: {L.tmdnet_last_error(st.handle).decode()} (code {rc})")
                if getattr(st, "pair_priors", False):  # this energy does not come through energy_and_forces: the priors are added here
                    self._add_pair_priors(st, stream, n, n_mol, p32, z, batch, box, box_mode, energy, None, None)
                st.ws_epoch = getattr(st, "ws_epoch", 0) + 1
                token["epoch"] = st.ws_epoch
        return energy, token

    def _train_backward(self, token, grad_energy):
        L = _C.lib()
        dev = token["dev"]
        z, batch, q, n, n_mol, n_pairs = token["z"], token["batch"], token["q"], token["n"], token["n_mol"], token["n_pairs"]
        with torch.cuda.device(dev):
            st = self._engine
            stream = _stream_ptr(dev)
            ge = grad_energy.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            assert ge.numel() == n_mol
            flat = torch.empty(token["grad_floats"], dtype=torch.float32, device=dev)
            kept = (token["epoch"] is not None and getattr(st, "ws_epoch", 0) == token["epoch"] and st.handle is not None
                    and st.handle.value == token["handle"])
            if not kept:  # the workspaces were reused (or never filled): rebuild the graph and run both halves
                _, fresh = self._train_forward(z, token["pos"], batch, token["box"], q, n_mol, keep=False)
                st = self._engine
                n_pairs = fresh["n_pairs"]
            rc = L.tmdnet_energy_param_grads(st.handle, stream, _ptr(st.graph_ws), _ptr(st.fwd_ws), st.fwd_ws.numel(),
                                             _ptr(st.train_ws), st.train_ws.numel(), n, n_mol, n_pairs, _ptr(z), _ptr(batch), _ptr(q),
                                             _ptr(ge), None if kept else _ptr(token["energy"]), _ptr(flat))
            if rc != _C.OK:
                raise RuntimeError(f"tmdnet_energy_param_grads: {L.tmdnet_last_error(st.handle).decode()} (code {rc})")
            if not kept and getattr(st, "pair_priors", False):  # the energies were written by this call: the priors are added here
                tb = token["box"]
                self._add_pair_priors(st, stream, n, n_mol, token["pos"], z, batch, tb, 0 if tb is None else (1 if tb.dim() == 2 else 2),
                                      token["energy"], None, None)
            st.ws_epoch = getattr(st, "ws_epoch", 0) + 1
            ent = {}
            for i in range(L.tmdnet_param_grad_count(st.handle)):
                off, numel = C.c_int64(0), C.c_int64(0)
                name = L.tmdnet_param_grad_entry(st.handle, i, C.byref(off), C.byref(numel)).decode()
                ent[name] = flat[off.value: off.value + numel.value]
            grads = self._et_grads(ent) if self._is_et() else (self._tn2_grads(ent) if self._is_tn2() else self._tensornet_grads(ent))
            if self.prior_model is not None:  # Atomref: E_m += sum_i atomref[z_i]
                for pr in self._atomref_priors():
                    if pr.enable:
                        w = pr.atomref.weight
                        grads[w] = torch.zeros(w.shape[0], dtype=torch.float32, device=dev).index_add_(0, z, ge[batch]).view_as(w)
        return grads

    def _tensornet_grads(self, ent, skip=()):
        grads = {p: ent[k].view_as(p) for k, p in self._grad_targets().items() if not k.endswith(skip)}
        te = self.representation_model.tensor_embedding
        F = te.emb.weight.shape[1]
        Wdp, bdp = ent["Wdp"].view(3, F, -1), ent["bdp"].view(3, F)
        for k, proj in enumerate((te.distance_proj1, te.distance_proj2, te.distance_proj3)):
            grads[proj.weight], grads[proj.bias] = Wdp[k], bdp[k]
        # species tables U[z] = emb[z] Wa^T + b, V[z] = emb[z] Wb^T with emb2.weight = [Wa | Wb] (reference tensornet.py:526-541)
        dU, dV = ent["Utab"].view(-1, F), ent["Vtab"].view(-1, F)
        emb, w2 = te.emb.weight.detach().float(), te.emb2.weight.detach().float()
        grads[te.emb.weight] = dU @ w2[:, :F] + dV @ w2[:, F:]
        grads[te.emb2.weight] = torch.cat([dU.t() @ emb, dV.t() @ emb], dim=1)
        grads[te.emb2.bias] = dU.sum(0)
        return grads

    def _tn2_grads(self, ent):
        """TensorNet2: TensorNet's entries, the first edge-MLP layer as its three column blocks [pair | target charges | source
        charges] (reference tensornet2.py:536-560), and the ChargePredict heads (:49-157)"""
        rm = self.representation_model
        grads = self._tensornet_grads(ent, skip=("M0",))
        for l, layer in enumerate(rm.layers):
            t = "l%d." % l
            w = layer.linears_scalar[0].weight
            F = w.shape[0]
            grads[w] = torch.cat([ent[t + "M0"].view(F, -1), ent[t + "M0b"].view(F, -1), ent[t + "M0c"].view(F, -1)], dim=1)
        heads = [rm.charge_predict_0] + list(rm.charge_predicts)
        for h, cp in enumerate(heads):
            c = "cp%d." % h
            mlp = cp.q_mlp.layers
            for key, prm in (("ln_w", cp.q_norm.weight), ("ln_b", cp.q_norm.bias), ("W1", mlp[0].weight), ("b1", mlp[0].bias),
                             ("W2", mlp[2].weight), ("b2", mlp[2].bias), ("W3", mlp[4].weight), ("b3", mlp[4].bias)):
                grads[prm] = ent[c + key].view_as(prm)
        return grads

    def _et_grads(self, ent):
        """engine entries -> Equivariant Transformer parameters (packing of csrc/tn_et_api.hip et_finalize: q | k | v stacked, the
        value-type rows regrouped from the reference's per-head [H][3][hd] order to thirds [3][F])"""
        rm, on = self.representation_model, self.output_model.output_network
        F, hd = rm.hidden_channels, rm.hidden_channels // rm.num_heads
        c = torch.arange(F)
        src = torch.cat([(c // hd) * 3 * hd + t * hd + c % hd for t in range(3)])  # state-dict row of engine row t * F + c

        def unthirds(g):  # engine rows [3F, ...] -> state-dict order
            out = torch.empty_like(g)
            out[src.to(g.device)] = g
            return out

        grads = {rm.embedding.weight: ent["emb"].view_as(rm.embedding.weight), rm.out_norm.weight: ent["lno_w"],
                 rm.out_norm.bias: ent["lno_b"]}
        ne = rm.neighbor_embedding
        if ne is not None:
            grads.update({ne.embedding.weight: ent["embN"].view_as(ne.embedding.weight), ne.distance_proj.weight: ent["Wn"].view(F, -1),
                          ne.distance_proj.bias: ent["bn"], ne.combine.weight: ent["Wc"].view(F, 2 * F), ne.combine.bias: ent["bc"]})
        for l, al in enumerate(rm.attention_layers):
            t = "l%d." % l
            W, b = ent[t + "Wqkv"].view(5 * F, F), ent[t + "bqkv"]
            grads.update({al.layernorm.weight: ent[t + "ln_w"], al.layernorm.bias: ent[t + "ln_b"], al.q_proj.weight: W[:F],
                          al.q_proj.bias: b[:F], al.k_proj.weight: W[F:2 * F], al.k_proj.bias: b[F:2 * F],
                          al.v_proj.weight: unthirds(W[2 * F:]), al.v_proj.bias: unthirds(b[2 * F:]),
                          al.vec_proj.weight: ent[t + "Wvp"].view(3 * F, F), al.o_proj.weight: ent[t + "Wo"].view(3 * F, F),
                          al.o_proj.bias: ent[t + "bo"]})
            if al.dk_proj is not None or al.dv_proj is not None:
                Wd, bd = ent[t + "Wdkv"], ent[t + "bdkv"]
                Wd = Wd.view(bd.numel(), -1)
                o = 0
                if al.dk_proj is not None:
                    grads[al.dk_proj.weight], grads[al.dk_proj.bias] = Wd[:F], bd[:F]
                    o = F
                if al.dv_proj is not None:
                    grads[al.dv_proj.weight], grads[al.dv_proj.bias] = unthirds(Wd[o:o + 3 * F]), unthirds(bd[o:o + 3 * F])
        F2 = F // 2
        b0, b1 = on[0], on[1]
        W1u = ent["W1u"].view(F + F2, F)
        w2 = torch.zeros_like(b1.update_net.layers[2].weight, dtype=torch.float32)
        w2[0] = ent["Wn2"]
        bb2 = torch.zeros_like(b1.update_net.layers[2].bias, dtype=torch.float32)
        bb2[0] = ent["bn2"][0]
        grads.update({b0.vec1_proj.weight: W1u[:F], b0.vec2_proj.weight: W1u[F:], b0.update_net.layers[0].weight: ent["Wm1"].view(F, 2 * F),
                      b0.update_net.layers[0].bias: ent["bm1"], b0.update_net.layers[2].weight: ent["Wm2"].view(F, F),
                      b0.update_net.layers[2].bias: ent["bm2"], b1.vec1_proj.weight: ent["W21"].view(F2, F2),
                      b1.update_net.layers[0].weight: ent["Wn1"].view(F2, F), b1.update_net.layers[0].bias: ent["bn1"],
                      b1.update_net.layers[2].weight: w2, b1.update_net.layers[2].bias: bb2})
        return grads

    def _grow(self, buf, nbytes, device):
        if buf is None or buf.numel() < nbytes or buf.device != device:
            self._engine.generation += 1
            return torch.empty(max(int(nbytes * 1.1), 256), dtype=torch.uint8, device=device)
        return buf

    @staticmethod
    def _check_input(t: Tensor, name: str, dev, dtypes):
        if t.device != dev:
            raise RuntimeError(f"torchmdnet_amd: `{name}` is on {t.device} but `pos` is on {dev}; all inputs must live on the "
                               "same AMD GPU (the HIP kernels receive raw device pointers)")
        if t.dtype not in dtypes:
            raise TypeError(f"torchmdnet_amd: `{name}` must have dtype {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")

    def _check_mass_index(self, z):
        """The reference's atomic_mass[z] raises IndexError for z >= len(atomic_mass); the graph phase checks z < max_z only.  Read
        back once per `z` tensor and version (an MD loop keeps its `z`: no synchronisation per step), never during a capture."""
        mass = getattr(self.output_model, "atomic_mass", None)
        if mass is None or mass.numel() >= self.representation_model.max_z or not z.numel():
            return
        key = (z.data_ptr(), z._version, tuple(z.shape))
        if getattr(self._engine, "mass_checked", None) == key or torch.cuda.is_current_stream_capturing():
            return
        zmax = int(z.max())
        if zmax >= mass.numel():
            raise IndexError(f"index {zmax} is out of bounds for the atomic mass table of size {mass.numel()}")
        self._engine.mass_checked = key

    def energy_and_forces(self, z, pos, batch, box, q, n_mol, want_forces=True, atom_weights=None,
                          halo_exchange=None, cell_grid=None, want_virial=False):
        """Raw engine call: returns (E [n_mol], F [N,3] or None), both fp32 on ``pos.device``.  ``atom_weights`` ([N] fp32, this
        framework's extension for domain decomposition, parallel.SpatialEvaluator): E_mol = sum_i w_i e_i + mean and F = -dE/dpos
        of that sum (TensorNet only).  ``halo_exchange(stage, rows, inv)`` (parallel.HaloExchangeEvaluator, TensorNet only) is
        called 2 L + 1 times inside the step (``tmdnet_set_halo_exchange``, include/tmdnet_amd.h): it overwrites the ghost rows of
        ``rows`` [N, row_floats] (a view of the engine's workspace) with their owners' values on the current stream; the row of
        the caller's atom i is ``rows[i]`` when ``inv`` is None and ``rows[inv[i]]`` otherwise (cell order).  ``cell_grid``
        (n_x, n_y, n_z) fixes the neighbour search's grid (``tmdnet_set_cell_grid``; default: from the box on the device).
        ``want_virial=True`` (TensorNet and Equivariant Transformer, scalar head) returns a third element W [n_mol,3,3], the virial
        W_m[a][b] = -dE_m/d eps_ab under pos -> pos (I + eps), box -> box (I + eps) (``tmdnet_energy_forces_virial``); E and F are
        bit-identical to the two-element call.  A model with a ZBL / D2 prior runs the pair pass behind the model's
        (``tmdnet_pair_priors_add``: three more launches on the same stream, E, F and W added in place; ``want_forces=False`` adds the
        energy only); without one nothing else is launched.  Pair priors refuse ``atom_weights`` and ``halo_exchange``."""
        _require_cuda(pos, "TorchMD_Net.forward")
        L = _C.lib()
        dev = pos.device
        pdev = next(self.parameters()).device
        if pdev != dev and pdev.type != "cpu":  # host-resident parameters are uploaded to the engine from the host (full upload)
            raise RuntimeError("model and inputs are on different devices")
        self._check_input(z, "z", dev, (torch.long,))
        self._check_input(batch, "batch", dev, (torch.long, torch.int32))
        if z.shape[0] != pos.shape[0] or batch.shape[0] != pos.shape[0]:
            raise ValueError(f"z [{z.shape[0]}], pos [{pos.shape[0]}] and batch [{batch.shape[0]}] must have one entry per atom")
        if want_virial:
            self._refuse_virial(atom_weights, halo_exchange)
            want_forces = True  # the virial is a by-product of the force pass
        if self.prior_model is not None and (atom_weights is not None or halo_exchange is not None):
            self._refuse_pair_priors("atom weights or the halo exchange (domain decomposition)")
        if self._head_kind() != _C.HEAD_SCALAR:
            if atom_weights is not None or halo_exchange is not None:
                raise NotImplementedError(f"{type(self.output_model).__name__}: atom weights and the halo exchange have no HIP path "
                                          "with a property head")
            self._check_mass_index(z)
        with torch.cuda.device(dev):
            st = self._sync_engine()
            stream = _stream_ptr(dev)
            n = int(z.shape[0])
            p32 = pos.detach().to(torch.float32).contiguous()
            z = z.contiguous()
            batch = batch.to(torch.long).contiguous()
            box_mode = 0
            if box is not None:
                box = box.detach().to(device=dev, dtype=torch.float32).contiguous()
                box_mode = 1 if box.dim() == 2 else 2
            if self._is_et():
                q = None  # TorchMD_ET.forward takes q / s and ignores them (torchmd_et.py:188-196)
            if q is not None:
                q = q.detach().to(device=dev, dtype=torch.float32).contiguous()
                if q.numel() != n_mol:
                    raise ValueError(f"q must have one entry per molecule ({n_mol}), got {q.numel()}")
            if getattr(st, "pair_priors", False):
                self._check_pair_prior_inputs(z, batch, n_mol)
            # neighbour strategy: O(N) cell list for one large system - periodic (grid computed on the device from the box of
            # THIS call: nothing about the box is cached on the host) or not (fictitious box around the bounding box, as the
            # reference's cell strategy, models/utils.py:206-212) -, brute force inside each molecule otherwise
            # ... or several LARGE molecules that share the box / the bounding box (interleaved in cell order inside the engine)
            auto = box_mode != 2 and n_mol >= 1 and n >= self.cell_list_min_atoms * n_mol
            grid = (-1, -1, -1) if auto else (0, 0, 0)
            if cell_grid is not None and auto:
                grid = tuple(int(v) for v in cell_grid)
            L.tmdnet_set_cell_grid(st.handle, *grid)
            # the atom weights and the exchange are set BEFORE the graph is built: with both, the cell list leaves out the pairs of two
            # ghosts (tmdnet_build_graph)
            if atom_weights is not None:
                atom_weights = atom_weights.detach().to(device=dev, dtype=torch.float32).contiguous()
                if atom_weights.numel() != n:
                    raise ValueError(f"atom_weights must have one entry per atom ({n}), got {atom_weights.numel()}")
            L.tmdnet_set_atom_weights(st.handle, _ptr(atom_weights))
            st.atom_weights = atom_weights
            if atom_weights is not None and torch.cuda.is_current_stream_capturing():
                # a captured graph replays the call with this pointer: the vector has to outlive every replay, and a later call
                # (which overwrites st.atom_weights) must not free it
                # (bounded: a re-capture with the same storage adds nothing, and only the most recent 8 captures are kept alive)
                kept = [w for w in getattr(st, "captured_atom_weights", []) if w.data_ptr() != atom_weights.data_ptr()]
                st.captured_atom_weights = (kept + [atom_weights])[-8:]
            halo_state = {}
            if halo_exchange is not None:

                def _halo(_user, stage, rows_ptr, n_rows, row_floats, perm_ptr, _stream):
                    try:  # an exception must not unwind through the C frames: kept, re-raised after the call
                        ws_t, g_t = st.fwd_ws, st.graph_ws  # grown after the graph is built
                        o = int(rows_ptr) - ws_t.data_ptr()
                        rows = ws_t[o:o + 4 * n_rows * row_floats].view(torch.float32).view(n_rows, row_floats)
                        if perm_ptr and "inv" not in halo_state:
                            po = int(perm_ptr) - g_t.data_ptr()
                            perm = g_t[po:po + 4 * n_rows].view(torch.int32).long()
                            inv = torch.empty_like(perm)
                            inv[perm] = torch.arange(n_rows, device=perm.device)
                            halo_state["inv"] = inv
                        halo_exchange(int(stage), rows, halo_state.get("inv"))
                        return 0
                    except BaseException as e:  # noqa: BLE001
                        halo_state["error"] = e
                        return 1

                halo_state["cb"] = _C.HALO_EXCHANGE_FN(_halo)
                L.tmdnet_set_halo_exchange(st.handle, halo_state["cb"], None)
            try:
                nbytes = C.c_size_t(0)
                L.tmdnet_graph_workspace_bytes(st.handle, n, n_mol, C.byref(nbytes))
                counts = (C.c_int64 * 8)()
                static = bool(getattr(self.representation_model, "static_shapes", False))
                st.graph_ws = self._grow(st.graph_ws, nbytes.value, dev)
                if static:
                    # static shapes (reference tensornet.py:277-290): no read-back, no synchronisation -> the whole call
                    # can be captured in a HIP graph; launch grids / workspaces are sized by max_num_neighbors * N
                    rc = L.tmdnet_build_graph_static(st.handle, stream, _ptr(st.graph_ws), st.graph_ws.numel(), n, n_mol, _ptr(p32),
                                                     _ptr(batch), _ptr(z), _ptr(box), box_mode)
                    n_pairs, n_edges = -1, -1
                else:
                    rc = L.tmdnet_build_graph(st.handle, stream, _ptr(st.graph_ws), st.graph_ws.numel(), n, n_mol, _ptr(p32),
                                              _ptr(batch), _ptr(z), _ptr(box), box_mode, counts)
                    n_pairs, n_edges = int(counts[0]), int(counts[1])
                    st.counts = (n_pairs, n_edges, int(counts[3]))
                    self._raise_bad_indices(counts, L.tmdnet_last_error(st.handle).decode())
                if rc == _C.ERR_OVERFLOW:
                    # same exception type and message as the reference (models/utils.py:297-300)
                    raise RuntimeError(L.tmdnet_last_error(st.handle).decode())
                if rc != _C.OK:
                    raise RuntimeError(f"tmdnet_build_graph: {L.tmdnet_last_error(st.handle).decode()} (code {rc})")
                L.tmdnet_forward_workspace_bytes(st.handle, n, n_mol, n_pairs, n_edges, int(want_forces), C.byref(nbytes))
                st.fwd_ws = self._grow(st.fwd_ws, nbytes.value, dev)
                # the vector output (EquivariantVectorOutput) has three components per molecule
                shape = (n_mol, 3) if self._head_kind() == _C.HEAD_VECTOR else (n_mol,)
                energy = torch.empty(shape, dtype=torch.float32, device=dev)
                forces = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_forces else None
                st.ws_epoch = getattr(st, "ws_epoch", 0) + 1  # the workspaces of a pending parameter-gradient pass are gone
                if want_virial:
                    L.tmdnet_virial_workspace_bytes(st.handle, n, n_mol, C.byref(nbytes))
                    if st.virial_ws is None:  # the first one: no captured graph can hold its address, the generation stays
                        st.virial_ws = torch.empty(max(int(nbytes.value * 1.1), 256), dtype=torch.uint8, device=dev)
                    st.virial_ws = self._grow(st.virial_ws, nbytes.value, dev)
                    virial = torch.empty((n_mol, 3, 3), dtype=torch.float32, device=dev)
                    rc = L.tmdnet_energy_forces_virial(st.handle, stream, _ptr(st.graph_ws), _ptr(st.fwd_ws), st.fwd_ws.numel(),
                                                       _ptr(st.virial_ws), st.virial_ws.numel(), n, n_mol, n_pairs, _ptr(z), _ptr(batch),
                                                       _ptr(q), 1, _ptr(energy), _ptr(forces), _ptr(virial))
                else:
                    rc = L.tmdnet_energy_forces(st.handle, stream, _ptr(st.graph_ws), _ptr(st.fwd_ws), st.fwd_ws.numel(), n, n_mol,
                                                n_pairs, _ptr(z), _ptr(batch), _ptr(q), int(want_forces), _ptr(energy), _ptr(forces))
                if rc == _C.OK and getattr(st, "pair_priors", False):
                    # ZBL / D2: one pair pass behind the model's, which adds to its outputs (same stream: ordered, capturable)
                    self._add_pair_priors(st, stream, n, n_mol, p32, z, batch, box, box_mode, energy, forces,
                                          virial if want_virial else None)
            finally:  # also when the graph phase raised: the handle must not keep a callback or weights that are about to be freed
                if halo_exchange is not None:
                    L.tmdnet_set_halo_exchange(st.handle, _C.HALO_EXCHANGE_FN(), None)
                if atom_weights is not None:
                    L.tmdnet_set_atom_weights(st.handle, None)
            if "error" in halo_state:
                raise halo_state["error"]
            if rc == _C.ERR_INVALID and want_virial:  # a refusal of the C entry that the checks above did not anticipate
                raise NotImplementedError(f"tmdnet_energy_forces_virial: {L.tmdnet_last_error(st.handle).decode()}")
            if rc != _C.OK:
                raise RuntimeError(f"tmdnet_energy_forces: {L.tmdnet_last_error(st.handle).decode()} (code {rc})")
            if static and self.static_check and not torch.cuda.is_current_stream_capturing():
                # outside a capture the overflow flag is polled (one sync); replays of a captured graph are unchecked,
                # like the reference's asynchronous assert (models/utils.py:297-300): call check_overflow() when convenient
                self.check_overflow(n, n_mol)
        if want_virial:
            return energy, forces, virial
        return energy, forces

    def _refuse_virial(self, atom_weights=None, halo_exchange=None):
        """What the virial is not implemented for (``tmdnet_energy_forces_virial`` answers TMDNET_ERR_INVALID for the same cases):
        raised before anything is set on the handle, which stays usable."""
        if self._is_tn2():
            raise NotImplementedError("the virial has no HIP path for TensorNet2: the Coulomb head's forces do not come from the "
                                      "per-pair gradient")
        if self._head_kind() != _C.HEAD_SCALAR:
            raise NotImplementedError(f"the virial has no HIP path with output_model {type(self.output_model).__name__} "
                                      "(scalar head only)")
        if atom_weights is not None or halo_exchange is not None:
            raise NotImplementedError("the virial has no HIP path with atom weights or the halo exchange")
        if self.parameter_gradients and torch.is_grad_enabled():
            raise NotImplementedError("the virial has no HIP path inside the parameter-gradient and second-order passes "
                                      "(parameter_gradients=True): evaluate it under torch.no_grad()")

    @staticmethod
    def stress(W: Tensor, box: Tensor) -> Tensor:
        """Stress of every molecule from its virial: sigma_m = -W_m / V_m with V_m = |det box_m|.  ``W`` [B,3,3] (or [3,3]), ``box``
        one [3,3] box for all molecules or one per molecule [B,3,3]."""
        vol = torch.linalg.det(box.to(device=W.device, dtype=W.dtype)).abs()
        return -W / (vol.reshape(-1, 1, 1) if box.dim() == 3 else vol)

    def energy_forces_virial(self, z: Tensor, pos: Tensor, batch: Optional[Tensor] = None, box: Optional[Tensor] = None,
                             q: Optional[Tensor] = None, num_systems: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """(E [B,1], F [N,3], W [B,3,3]): energies, forces and the virial W_m[a][b] = -dE_m/d eps_ab under the homogeneous strain
        pos -> pos (I + eps), box -> box (I + eps) (row vectors; ``stress(W, box)`` = -W / V).  Inputs are staged and checked as in
        ``forward``; E and F are bit-identical to ``forward``'s.  When ``pos`` or ``box`` requires grad, the call goes through the
        registered operator ``tmdnet::energy_forces_virial``: ``E.backward()`` then fills ``pos.grad`` (from F) and ``box.grad``
        (from W and F); F and W themselves carry no graph (second derivatives raise)."""
        assert z.dim() == 1 and z.dtype == torch.long
        batch = torch.zeros_like(z) if batch is None else batch
        if pos.dtype != torch.float32:
            raise NotImplementedError("torchmdnet_amd computes in fp32; cast positions to float32")
        if pos.device.type == "cpu" and torch.cuda.is_available():  # host tensors: staged as in _forward_host_tensors
            dev = torch.device("cuda", torch.cuda.current_device())
            pdev = next(self.parameters()).device
            if pdev.type == "cuda":
                dev = pdev
            mv = lambda t: None if t is None else t.to(dev)
            e, f, w = self.energy_forces_virial(z.to(dev), pos.to(dev), mv(batch), mv(box), mv(q), num_systems)
            return e.to(pos.device), f.to(pos.device), w.to(pos.device)
        _require_cuda(pos, "TorchMD_Net.energy_forces_virial")
        n_mol = int(num_systems) if num_systems is not None else (int(batch.max().item()) + 1 if z.numel() else 0)
        rm = self.representation_model
        if box is None and rm.distance.use_periodic:
            box = rm.distance.box
        if box is not None and box.device != pos.device:
            box = box.to(pos.device)
        self._refuse_virial()
        grad = torch.is_grad_enabled() and (pos.requires_grad or (box is not None and box.requires_grad))
        if grad:
            if self._engine.op_key is None:
                self._engine.op_key = ops.register_engine(self)
            energy, forces, virial = torch.ops.tmdnet.energy_forces_virial(z, pos, batch, box, q, self._engine.op_key, n_mol)
        else:
            energy, forces, virial = self.energy_and_forces(z, pos, batch, box, q, n_mol, want_virial=True)
        return energy.view(-1, 1), forces, virial

    @staticmethod
    def _raise_bad_indices(counts, msg):
        if int(counts[5]):  # the reference's scatter over `batch` raises a RuntimeError for an index outside [0, dim_size)
            raise RuntimeError(msg)
        if int(counts[4]):  # nn.Embedding raises IndexError (tensornet.py:473, torchmd_et.py:144)
            raise IndexError(msg)

    def check_overflow(self, n_atoms: int, n_mol: int):
        """Poll the device-side pair counters of the last static-shape evaluation (synchronises)."""
        L = _C.lib()
        st = self._engine
        counts = (C.c_int64 * 8)()
        rc = L.tmdnet_graph_counts(st.handle, _stream_ptr(st.graph_ws.device), _ptr(st.graph_ws), n_atoms, n_mol, counts)
        st.counts = (int(counts[0]), int(counts[1]), int(counts[3]))
        self._raise_bad_indices(counts, L.tmdnet_last_error(st.handle).decode())
        if rc == _C.ERR_OVERFLOW:
            raise RuntimeError("Found num_pairs > max_num_pairs, please increase max_num_pairs "
                               f"(found {int(counts[1])} edges for max_num_neighbors={self.representation_model.max_num_neighbors})")
        return st.counts

    def graph_counts(self):
        """(pairs P, directed edges incl. self loops E, 1 if `batch` was not sorted) of the last graph the host read back: every dynamic-shape
        evaluation and ``check_overflow``; None before the first.  ``debug_tensor("dkv<l>", (P + 1, Wd))`` takes its P from here."""
        return self._engine.counts

    def engine_info(self, name: str) -> float:
        """Library-side facts about the uploaded model, e.g. "edge_table_T" (0: radial tables off), "edge_table_err_value"."""
        st = self._sync_engine()
        v = C.c_double(0.0)
        if _C.lib().tmdnet_get_info(st.handle, name.encode(), C.byref(v)) != _C.OK:
            raise KeyError(name)
        return v.value

    def set_engine_option(self, name: str, value: float):
        """Library-side switches, e.g. ("edge_table_min_pairs", n): systems with fewer pairs run the pair-row GEMMs directly."""
        st = self._sync_engine()
        self._engine.options = dict(getattr(self._engine, "options", {}), **{name: float(value)})
        if _C.lib().tmdnet_set_option(st.handle, name.encode(), float(value)) != _C.OK:
            raise KeyError(name)

    def cell_grid(self, n_atoms: int, n_mol: int = 1):
        """(n_x, n_y, n_z, used) of the last evaluation's neighbour search; used = 0: brute force ran (synchronises)."""
        L = _C.lib()
        st = self._engine
        grid = (C.c_int64 * 4)()
        L.tmdnet_graph_cell_grid(st.handle, _stream_ptr(st.graph_ws.device), _ptr(st.graph_ws), n_atoms, n_mol, grid)
        return tuple(int(v) for v in grid)

    def _capture_inputs(self, name, needs, z, pos, batch, box, q, num_systems, steps_per_replay=1, atom_weights=None,
                        halo_exchange=None, box_moves=False, coords="positions"):
        """The prelude of every ``capture*`` method ``name``: what no captured graph can serve is refused, then the inputs are staged.
        ``needs`` is the loop's noun phrase ("a band needs"); None: ``capture`` itself, which serves every head, training models and
        whatever ``energy_and_forces`` takes as positions.  -> (z, batch, box, q, n_mol, dev)

        The graph records raw device pointers of EVERY input.  They are brought to the device / dtype the engine takes HERE (inside
        energy_and_forces a conversion would be a temporary) and whoever holds the graph keeps them alive (``inputs``): before this
        rule a caller that passed temporaries (z.cuda(), an int32 batch, ...) replayed over freed memory.  A box that needs no
        conversion stays the caller's own object, so that in-place updates remain visible to the graph and a loop's ``box`` IS the
        tensor the caller scales or reads.  ``box_moves``: the graph also WRITES the box (a barostat, a cell relaxation), so the
        model's own box is cloned first: it stays as it was created."""
        if not getattr(self.representation_model, "static_shapes", False):
            raise RuntimeError(f"{name}() needs a model created with static_shapes=True")
        if needs is not None and self._head_kind() != _C.HEAD_SCALAR:
            raise NotImplementedError(f"{name} has no HIP path with output_model {type(self.output_model).__name__}: {needs} energies "
                                      "and their forces (scalar head)")
        if needs is not None and self.parameter_gradients:
            raise NotImplementedError(f"{name} has no HIP path with parameter_gradients=True (a training model); create the model "
                                      "without it")
        if atom_weights is not None or halo_exchange is not None:
            raise NotImplementedError(f"{name} has no HIP path with atom weights or the halo exchange (domain decomposition)")
        if int(steps_per_replay) < 1:
            raise ValueError(f"steps_per_replay must be at least 1, got {steps_per_replay}")
        _require_cuda(pos, name)
        if needs is not None and pos.dtype != torch.float32:
            raise NotImplementedError(f"torchmdnet_amd computes in fp32; cast {coords} to float32")
        batch = torch.zeros_like(z) if batch is None else batch
        n_mol = int(num_systems) if num_systems is not None else int(batch.max().item()) + 1
        rm = self.representation_model
        if box is None and rm.distance.use_periodic:
            box = rm.distance.box
        dev = pos.device
        z = z.detach().to(device=dev, dtype=torch.long).contiguous()
        batch = batch.detach().to(device=dev, dtype=torch.long).contiguous()
        q = None if q is None else q.detach().to(device=dev, dtype=torch.float32).contiguous()
        if box is not None:
            if box_moves and box is getattr(rm.distance, "box", None):
                box = box.clone()
            staged = box.detach().to(device=dev, dtype=torch.float32).contiguous()
            box = box if staged.data_ptr() == box.data_ptr() and not box.requires_grad else staged
        return z, batch, box, q, n_mol, dev

    def capture(self, z: Tensor, pos: Tensor, batch: Optional[Tensor] = None, box: Optional[Tensor] = None,
                q: Optional[Tensor] = None, num_systems: Optional[int] = None, warmup: int = 3, virial: bool = False):
        """Capture one energy+force evaluation into a HIP graph (needs ``static_shapes=True``).  ``virial=True``: the graph also
        computes the virial; the replay then returns ``(energy, forces, W [B,3,3])`` and ``replay.virial`` is the static W buffer.
        Returns ``replay(pos) -> (energy [B,1] ([B,3]: vector output), forces [N,3])`` writing into static buffers - the reference gets
        the same effect with torch.cuda.graphs around its model (calculators.py:117-128)."""
        z, batch, box, q, n_mol, dev = self._capture_inputs("capture", None, z, pos, batch, box, q, num_systems)
        s_pos = pos.detach().clone().contiguous()
        out = []

        def evaluate():
            if virial:
                return self.energy_and_forces(z, s_pos, batch, box, q, n_mol, want_forces=True, want_virial=True)
            return self.energy_and_forces(z, s_pos, batch, box, q, n_mol, want_forces=True)

        graph = captured.capture_graph(dev, evaluate, lambda: out.extend(evaluate()), warmup)
        s_e, s_f, s_w = out if virial else (*out, None)
        token = captured.engine_token(self)

        def replay(new_pos: Optional[Tensor] = None):
            captured.check_fresh(captured.engine_token(self), token, "capture()")
            if new_pos is not None:
                # an elementwise kernel, not Tensor.copy_: a same-dtype device copy goes through the runtime's blit path, which
                # costs ~3x a small kernel between two graph launches.  Integrators that can write in place use replay.pos.
                torch.mul(new_pos.detach(), 1.0, out=s_pos)
            graph.replay()
            if s_w is not None:
                return s_e.view(-1, 1), s_f, s_w
            return (s_e.view(-1, 3) if s_e.dim() == 2 else s_e.view(-1, 1)), s_f

        replay.graph = graph
        replay.inputs = (z, batch, box, q)  # what the graph reads, kept alive for as long as it can be replayed
        replay.pos = s_pos  # the positions the graph reads: write them in place and call replay() to skip the copy
        replay.n_atoms, replay.n_mol = int(z.shape[0]), n_mol
        if s_w is not None:
            replay.virial = s_w  # static buffer the graph writes W into
        return replay

    def capture_md(self, z: Tensor, pos: Tensor, vel: Tensor, masses: Tensor, dt: float, batch: Optional[Tensor] = None,
                   box: Optional[Tensor] = None, q: Optional[Tensor] = None, num_systems: Optional[int] = None,
                   steps_per_replay: int = 10, force_scale: float = 1.0, thermostat: Optional[dict] = None, warmup: int = 3,
                   atom_weights=None, halo_exchange=None, barostat: Optional[dict] = None):
        """Capture ``steps_per_replay`` full MD steps into ONE HIP graph (needs ``static_shapes=True``): per step half-kick, drift,
        neighbour list + energy + forces, half-kick, the Langevin O step when ``thermostat=dict(friction=, kT=, seed=)`` is given, and
        the energy bookkeeping, with the integrator as HIP kernels between the evaluations (``tmdnet_md_advance``) - no host work
        between steps.  ``masses`` [N]; per atom hk = dt force_scale / (2 m) and sigma = sqrt(kT force_scale / m), so ``force_scale``
        converts force / mass into length / time^2: 9.648533e-3 for eV, Angstrom, amu and fs (``md.FORCE_SCALE_EV_A_AMU_FS``).
        Positions are never wrapped.  Works for every architecture ``capture`` serves and for a batch of independent replicas.
        Returns a ``torchmdnet_amd.md.DeviceMD``: ``md(n)`` replays n times; ``md.pos / vel / forces``, ``md.epot / ekin`` [K,B],
        ``md.steps_done``, ``md.check()``, ``md.reset(pos, vel, step)``.  Inputs are staged and kept alive as in ``capture``; a ``box``
        that needs no conversion stays the caller's object.  ``atom_weights`` / ``halo_exchange`` are accepted only to be refused.
        ``barostat=dict(pressure=, tau=, compressibility=, kT=, seed=)`` (NPT): after every step an isotropic stochastic-cell-rescaling
        move per molecule scales ``md.box``, positions and velocities inside the graph (``tmdnet_md_barostat``), from the virial
        of that step's evaluation; pressure in E / length^3 (``md.BAR_IN_EV_PER_A3``), compressibility in length^3 / E, ``kT``
        (default: the thermostat's; 0 = weak coupling) in E, ``seed`` default the thermostat's.  Needs a box per molecule ([3,3] for
        one molecule, [B,3,3] otherwise) and an architecture with a virial (not TensorNet2); logs in ``md.volume / pressure /
        scale`` [K,B].
        Distance constraints (X-H bonds, rigid water): ``capture_md_constrained``, the same call with ``constraints=`` after these."""
        return self.capture_md_constrained(z, pos, vel, masses, dt, batch, box, q, num_systems, steps_per_replay, force_scale,
                                           thermostat, warmup, atom_weights, halo_exchange, barostat, None)

    def capture_md_constrained(self, z: Tensor, pos: Tensor, vel: Tensor, masses: Tensor, dt: float, batch: Optional[Tensor] = None,
                               box: Optional[Tensor] = None, q: Optional[Tensor] = None, num_systems: Optional[int] = None,
                               steps_per_replay: int = 10, force_scale: float = 1.0, thermostat: Optional[dict] = None,
                               warmup: int = 3, atom_weights=None, halo_exchange=None, barostat: Optional[dict] = None,
                               constraints: Optional[dict] = None):
        """``capture_md`` - its parameters in its order, with its meaning - plus ``constraints`` after them (None: ``capture_md``).
        ``constraints=dict(pairs=, lengths=None, tol=1e-6, max_iter=64)``: holonomic distance constraints |x_i - x_j| = d by RATTLE
        inside the graph (``tmdnet_md_advance_constrained``) - SHAKE after the drift, the velocity projection after the closing kick,
        still one integrator launch between two evaluations.  ``pairs`` [C,2] int64 in the caller's atom order (``md.hydrogen_pairs``
        makes them for X-H bonds and rigid water), ``lengths`` [C] (None: measured from ``pos`` in fp64).  The coupled constraints of
        one cluster are limited to 8 atoms and 12 constraints; ``pos`` must satisfy the constraints; ``vel`` is projected onto them.
        Every architecture; not together with ``barostat`` (the constraint forces' virial is not built).  ``md.constraints``,
        ``md.ndof`` [B]; ``md.check()`` raises when an iteration did not converge."""
        return self._capture_md(z, pos, vel, masses, dt, batch, box, q, num_systems, steps_per_replay, force_scale, thermostat, warmup,
                                atom_weights, halo_exchange, barostat, constraints, None)

    def capture_md_biased(self, z: Tensor, pos: Tensor, vel: Tensor, masses: Tensor, dt: float, batch: Optional[Tensor] = None,
                          box: Optional[Tensor] = None, q: Optional[Tensor] = None, num_systems: Optional[int] = None,
                          steps_per_replay: int = 10, force_scale: float = 1.0, thermostat: Optional[dict] = None, warmup: int = 3,
                          atom_weights=None, halo_exchange=None, barostat: Optional[dict] = None, constraints: Optional[dict] = None,
                          bias: Optional[dict] = None):
        """``capture_md`` - its parameters in its order, with its meaning - plus ``bias``: collective-variable restraints and
        metadynamics inside the graph (``tmdnet_md_bias``: one launch per step, between the evaluation and the integrator launch, adds
        the bias force to the model's force).  The B molecules of the batch are walkers.
        ``bias=dict(cvs=, restraints=, metad=, log_forces=False)``:
        ``cvs=[("distance", i, j), ("angle", i, j, k), ("torsion", i, j, k, l), ...]``, at most 8, indices relative to each
        molecule's first atom (``batch`` must be sorted), on the unwrapped positions without minimum image;
        ``restraints=[dict(cv=, kind="harmonic" | "upper" | "lower", kappa=, center=)]``, V = kappa / 2 (s - center)^2, ``kappa`` and
        ``center`` scalars or [B] - umbrella windows are one batch;
        ``metad=dict(cvs=[...], sigma=[...], height=, pace=, kT=, bias_factor=None, walkers_per_group=1, capacity=)`` on 1 or 2 of
        the CVs: every ``pace`` steps each walker deposits a Gaussian hill; consecutive walkers form groups of
        ``walkers_per_group`` that share one list of ``capacity`` hills; ``bias_factor`` gamma > 1 is well-tempered (None: plain).
        Every architecture ``capture_md`` serves; ``barostat`` and ``constraints`` are refused (the bias forces' virial and the
        constrained opening half are not wired in).  Returns a ``torchmdnet_amd.md.DeviceBiasedMD``: ``DeviceMD``'s surface
        (``forces`` is the total force) plus ``cv`` [K,B,D], ``restraint_energy`` / ``bias_energy`` [K,B], ``n_hills``, ``hills()``,
        ``bias_potential(s)``, ``free_energy(s)`` and ``reset(pos, vel, step, hills="keep" | "clear" | (centres, heights))``."""
        if bias is None:
            raise ValueError("capture_md_biased needs bias=dict(cvs=, restraints=, metad=); without a bias use capture_md")
        if barostat is not None:
            raise NotImplementedError("capture_md_biased has no HIP path with a barostat: the virial of the bias forces is not built")
        if constraints is not None:
            raise NotImplementedError("capture_md_biased has no HIP path with constraints: the bias launch is not wired into the "
                                      "constrained integrator")
        return self._capture_md(z, pos, vel, masses, dt, batch, box, q, num_systems, steps_per_replay, force_scale, thermostat, warmup,
                                atom_weights, halo_exchange, None, None, bias)

    def _capture_md(self, z, pos, vel, masses, dt, batch, box, q, num_systems, steps_per_replay, force_scale, thermostat, warmup,
                    atom_weights, halo_exchange, barostat, constraints, bias):
        from torchmdnet_amd.md import DeviceBiasedMD, DeviceMD, parse_barostat, prepare_bias, prepare_constraints

        if constraints is not None and barostat is not None:
            raise NotImplementedError("capture_md has no HIP path with constraints and a barostat together: the virial of the "
                                      "constraint forces is not built")
        z, batch, box, q, n_mol, _ = self._capture_inputs("capture_md", "molecular dynamics needs", z, pos, batch, box, q, num_systems,
                                                          steps_per_replay, atom_weights, halo_exchange, box_moves=barostat is not None)
        if barostat is not None:  # everything below is refused before anything is allocated or captured
            parse_barostat(barostat, thermostat)
            self._refuse_virial()
            if box is None:
                raise ValueError("capture_md(barostat=...) needs a box: the barostat scales it")
            if box.dim() == 2 and n_mol > 1:
                raise NotImplementedError("capture_md(barostat=...) has one barostat per molecule: give every molecule its own box "
                                          f"[{n_mol},3,3], not one shared [3,3] box")
        if constraints is not None:
            constraints = prepare_constraints(constraints, pos, batch, masses, n_mol)
        if bias is not None:
            bias = prepare_bias(bias, batch, z.shape[0], n_mol)
            return DeviceBiasedMD(self, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, thermostat, warmup,
                                  bias)
        return DeviceMD(self, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, thermostat, warmup,
                        barostat, constraints)

    def capture_md_global(self, z: Tensor, pos: Tensor, vel: Tensor, masses: Tensor, dt: float, batch: Optional[Tensor] = None,
                          box: Optional[Tensor] = None, q: Optional[Tensor] = None, num_systems: Optional[int] = None,
                          steps_per_replay: int = 10, force_scale: float = 1.0, warmup: int = 3, thermostat: Optional[dict] = None,
                          constraints: Optional[dict] = None):
        """``capture_md`` with a GLOBAL thermostat in place of the Langevin O step: after the closing kick of every step all
        velocities of a molecule are multiplied by ONE factor alpha computed from the molecule's kinetic energy inside the graph
        (``tmdnet_md_thermostat``: two launches), so the relative motion of the atoms - diffusion, vibrational spectra, relaxation
        times - is not damped.  One thermostat per molecule: a batch of B molecules is B independent thermostatted systems.
        ``thermostat=dict(kind="csvr", kT=, tau=, seed=0, ndof=None)``: stochastic velocity rescaling (Bussi, Donadio, Parrinello
        2007), canonical, noise a function of (seed, step, molecule);
        ``thermostat=dict(kind="nose-hoover", kT=, tau=, chain=3, substeps=2, ndof=None)``: a Nose-Hoover chain of 1..8 thermostats
        (Martyna, Klein, Tuckerman 1992), deterministic, ``substeps`` applications of the chain routine per step.
        ``kT`` in the unit of the energies, ``tau`` in the unit of ``dt``.  ``ndof`` (an int or [B]) defaults to ``md.ndof``: three per
        atom of finite mass minus the constraints; pass it after removing the centre-of-mass momentum.  A molecule with ``ndof == 0``
        or no kinetic energy is never scaled.  ``constraints=`` is the dict of ``capture_md_constrained``: a uniform scaling keeps
        the velocities on the constraints; the opening half is then a launch of its own.
        Returns a ``torchmdnet_amd.md.DeviceGlobalMD``: ``DeviceMD``'s surface plus ``scale`` [K,B], ``reservoir`` [K,B] float64,
        ``chain`` [B,2,M], ``kinetic_after()`` and ``conserved()``; ``ekin`` is the kinetic energy BEFORE each step's move.
        ``check()`` names the thermostat when a move was unusable (status 5); ``reset`` empties the thermostat.
        Not offered, so not parameters of this method (follow-ups): a barostat (MTK NPT), a bias, replica exchange, atom weights
        and the halo exchange.  Everything ``capture_md`` refuses is refused."""
        from torchmdnet_amd.md import DeviceGlobalMD, count_ndof, parse_global_thermostat, prepare_constraints, stage_ndof

        th = parse_global_thermostat(thermostat)  # everything below is refused before anything is allocated or captured
        z, batch, box, q, n_mol, _ = self._capture_inputs("capture_md_global", "molecular dynamics needs", z, pos, batch, box, q,
                                                          num_systems, steps_per_replay)
        if constraints is not None:
            constraints = prepare_constraints(constraints, pos, batch, masses, n_mol)
        stage_ndof(th["ndof"], count_ndof(masses, batch, n_mol, constraints), n_mol)
        return DeviceGlobalMD(self, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, warmup, th, constraints)

    def capture_md_observed(self, z: Tensor, pos: Tensor, vel: Tensor, masses: Tensor, dt: float, batch: Optional[Tensor] = None,
                            box: Optional[Tensor] = None, q: Optional[Tensor] = None, num_systems: Optional[int] = None,
                            steps_per_replay: int = 10, force_scale: float = 1.0, thermostat: Optional[dict] = None, warmup: int = 3,
                            constraints: Optional[dict] = None, observe: Optional[dict] = None):
        """``capture_md`` that records what happens between two replays: sample frames, the radial distribution function, the
        mean-square displacement and the velocity autocorrelation, inside the graph (``tmdnet_md_observe``: at most three launches
        after the evaluation of a SAMPLED step, none at any other step).  The observer reads ``pos`` / ``vel`` and writes only its own
        workspace: the trajectory is bit for bit that of the loop without it.
        ``thermostat``: None (NVE), the Langevin dict of ``capture_md``, or a dict with ``kind=`` ("csvr" / "nose-hoover"), which
        selects the loop of ``capture_md_global``.  ``constraints``: the dict of ``capture_md_constrained``.
        ``observe=dict(every=S, frames=, rdf=, msd=, vacf=)`` with at least one observable; ``S`` must divide ``steps_per_replay``.
        Samples are the steps s0 + S, s0 + 2 S, ... after the step s0 of the capture or the last ``reset``.
        ``frames=dict(capacity=F, velocities=False)``: a ring of the last F sampled frames -> ``md.frames()``;
        ``rdf=dict(pairs=[(za, zb), ...], r_max=, bins=)``: 1 to 4 pair types (None: every species), bins <= 1024, per molecule a
        histogram of pair distances over all samples (minimum image with a box; ``r_max`` at most half the smallest box height; the
        batch must be sorted) -> ``md.rdf()``;
        ``msd=dict(groups=[z | None, ...], capacity=T)``: sum |x(s) - x(s0)|^2 per sample, molecule and group from the unwrapped
        positions, T rows -> ``md.msd()``;
        ``vacf=dict(lags=L, groups=[...])``: L <= 256 lags of the autocorrelation of the leapfrog velocities v(s - 1/2) -> ``md.vacf()``.
        Returns the loop object of the chosen integrator (``DeviceMD`` or ``DeviceGlobalMD``) with the observer attached:
        ``md.n_samples`` and ``md.reset(..., observables="clear" | "keep")`` besides the four accessors.
        Not offered, so not parameters of this method (follow-ups): a barostat, a bias, replica exchange, atom weights and the halo
        exchange.  Everything ``capture_md`` refuses is refused, before anything is staged."""
        from torchmdnet_amd.md import DeviceGlobalMD, DeviceMD, count_ndof, parse_global_thermostat, prepare_constraints, stage_ndof
        from torchmdnet_amd.observe import Observer, parse_observe, prepare_observe

        parse_observe(observe, steps_per_replay)  # everything below is refused before anything is allocated or captured
        glob = thermostat is not None and "kind" in thermostat
        th = parse_global_thermostat(thermostat) if glob else thermostat
        z, batch, box, q, n_mol, dev = self._capture_inputs("capture_md_observed", "molecular dynamics needs", z, pos, batch, box, q,
                                                            num_systems, steps_per_replay)
        prep = prepare_observe(observe, z, batch, box, n_mol, steps_per_replay)
        if constraints is not None:
            constraints = prepare_constraints(constraints, pos, batch, masses, n_mol)
        if glob:
            stage_ndof(th["ndof"], count_ndof(masses, batch, n_mol, constraints), n_mol)
        observer = Observer(prep, z.shape[0], n_mol, dt, dev)
        if glob:
            return DeviceGlobalMD(self, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, warmup, th,
                                  constraints, observer)
        return DeviceMD(self, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, th, warmup, None,
                        constraints, observer)

    def capture_md_cell(self, z: Tensor, pos: Tensor, vel: Tensor, masses: Tensor, dt: float, batch: Optional[Tensor] = None,
                        box: Optional[Tensor] = None, q: Optional[Tensor] = None, num_systems: Optional[int] = None,
                        steps_per_replay: int = 10, force_scale: float = 1.0, thermostat: Optional[dict] = None, warmup: int = 3,
                        barostat: Optional[dict] = None):
        """``capture_md`` at constant pressure with a cell whose SHAPE fluctuates (crystals, slabs, membranes, solid-solid
        transitions): after every step an anisotropic stochastic-cell-rescaling move per molecule (Bernetti and Bussi 2020, written in
        the exponent) multiplies ``md.box`` and the positions by a 3 x 3 matrix mu = exp(D) and the velocities by exp(-D^T) inside the
        graph (``tmdnet_md_barostat_cell``: three launches after the closing half), from the full virial of that step's evaluation and
        the kinetic tensor.  ``barostat=dict(pressure=, tau=, compressibility=, kT=, seed=, coupling=, axis=2)``: the keys of
        ``capture_md``'s barostat with their units and defaults, plus ``coupling``:
        ``"anisotropic"`` (default) all nine entries of D; the box is kept lower triangular by rotating the whole system (positions,
        velocities and the forces of the last evaluation) with it;
        ``"diagonal"`` the three box lengths move independently, the angles stay;
        ``"semi-isotropic"`` ``axis`` moves on its own and the other two lengths share one strain (slabs and membranes).
        The target is hydrostatic (``pressure`` times the identity); ``kT=0`` is anisotropic weak coupling.  ``thermostat`` is the
        Langevin dict of ``capture_md`` or None.  Needs a box per molecule ([3,3] for one molecule, [B,3,3] otherwise) and an
        architecture with a virial (TensorNet, Equivariant Transformer; scalar head).  There is no lattice reduction: the minimum image
        is exact only while the box's off-diagonal entries stay below half its diagonal ones.
        Returns a ``torchmdnet_amd.md.DeviceCellMD``: ``DeviceMD``'s surface plus ``md.box``, ``md.volume`` [K,B],
        ``md.pressure_tensor`` [K,B,3,3], ``md.scale`` [K,B,3,3] and ``md.reset(pos=, vel=, box=)``; ``md.check()`` names the cell barostat
        when a move was unusable.  Not offered, so not parameters of this method: constraints, a bias, replica exchange, global
        thermostats, atom weights and the halo exchange."""
        from torchmdnet_amd.md import DeviceCellMD, parse_cell_barostat

        baro = parse_cell_barostat(barostat, thermostat)  # everything below is refused before anything is allocated or captured
        self._refuse_virial()
        z, batch, box, q, n_mol, _ = self._capture_inputs("capture_md_cell", "molecular dynamics needs", z, pos, batch, box, q, num_systems,
                                                          steps_per_replay, box_moves=True)
        if box is None:
            raise ValueError("capture_md_cell needs a box: the barostat moves it")
        if box.dim() == 2 and n_mol > 1:
            raise NotImplementedError("capture_md_cell has one barostat per molecule: give every molecule its own box "
                                      f"[{n_mol},3,3], not one shared [3,3] box")
        return DeviceCellMD(self, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, thermostat, warmup, baro)

    def capture_remd(self, z: Tensor, pos: Tensor, vel: Optional[Tensor], masses: Tensor, dt: float, temperatures=None,
                     exchange_every: int = 100, box: Optional[Tensor] = None, q: Optional[Tensor] = None, steps_per_replay: int = 100,
                     force_scale: float = 1.0, thermostat: Optional[dict] = None, warmup: int = 3, atom_weights=None,
                     halo_exchange=None, barostat=None, constraints=None):
        """Temperature replica exchange (parallel tempering) inside the captured MD graph: ``capture_md`` for B = G R replicas of ONE
        system - ``z`` [n], ``masses`` [n], ``pos`` [R,n,3] (one ladder) or [G,R,n,3] (G independent ladders), ``vel`` the same shape
        or None (Maxwell-Boltzmann velocities at each slot's kT, drawn on the host from the thermostat's seed) - where replica
        b = g R + r starts at ``temperatures[r]`` ([R] kT, in the unit of the energies; ``md.geometric_ladder``) and, after every
        ``exchange_every`` steps, neighbouring slots try to swap their TEMPERATURES by the Metropolis rule on the step's potential
        energies (``tmdnet_md_exchange``: two small launches between the closing and the opening half of the step; positions never
        move between replicas).  ``steps_per_replay`` must be a multiple of ``exchange_every``; ``exchange_every=0`` captures plain
        multi-temperature MD with no exchange launches.  ``thermostat=dict(friction=, seed=)`` is required (kT comes from
        ``temperatures``).  ``box`` [3,3] is shared, ``q`` holds one entry per ladder.  Every architecture ``capture_md`` serves;
        ``barostat``, ``constraints``, ``atom_weights`` and ``halo_exchange`` are refused.  Returns a ``torchmdnet_amd.md.DeviceREMD``:
        ``DeviceMD``'s surface plus ``slot`` [B], ``holder`` [G,R], ``slot_log`` [K/X,B], ``accepted`` [K/X,G,R-1], ``attempts`` /
        ``accepts`` [G,R-1], ``acceptance()``, ``temperatures``, ``by_slot(t)`` and ``reset(pos, vel, step, slots)``."""
        from torchmdnet_amd.md import DeviceREMD

        for name, val in (("barostat", barostat), ("constraints", constraints), ("atom_weights", atom_weights),
                          ("halo_exchange", halo_exchange)):
            if val is not None:
                raise ValueError(f"capture_remd has no path with {name}: neither the virial of the scaled state nor the constrained "
                                 "opening half is wired into the exchange")
        if thermostat is None:
            raise ValueError("capture_remd needs thermostat=dict(friction=, seed=): the temperatures act through the Langevin O step")
        if "kT" in thermostat:
            raise ValueError("capture_remd: the thermostat takes no 'kT'; give the ladder as temperatures=[R] kT")
        unknown = set(thermostat) - {"friction", "seed"}
        if unknown or "friction" not in thermostat:
            raise ValueError(f"capture_remd: thermostat=dict(friction=, seed=), got keys {sorted(thermostat)}")
        if temperatures is None:
            raise ValueError("capture_remd needs temperatures=[R] kT")
        kT = torch.as_tensor(temperatures, dtype=torch.float64).detach().cpu().reshape(-1)
        R = int(kT.numel())
        if R < 2 or not bool((torch.isfinite(kT) & (kT > 0)).all()):
            raise ValueError(f"capture_remd: temperatures must be at least two positive kT, got {kT.tolist()}")
        K, X = int(steps_per_replay), int(exchange_every)
        if K < 1 or X < 0:
            raise ValueError(f"capture_remd: steps_per_replay must be at least 1 and exchange_every at least 0, got {K}, {X}")
        if X and K % X:
            raise ValueError(f"capture_remd: steps_per_replay ({K}) must be a multiple of exchange_every ({X})")
        n = int(z.shape[0])
        if z.dim() != 1 or pos.dim() not in (3, 4) or tuple(pos.shape[-3:]) != (R, n, 3):
            raise ValueError(f"capture_remd: pos must be [R,n,3] = [{R},{n},3] or [G,{R},{n},3], got {tuple(pos.shape)}")
        if vel is not None and vel.shape != pos.shape:
            raise ValueError(f"capture_remd: vel {tuple(vel.shape)} must have the shape of pos {tuple(pos.shape)}")
        if masses.numel() != n:
            raise ValueError(f"capture_remd: masses must have one entry per atom of the system ({n}), got {masses.numel()}")
        G = int(pos.shape[0]) if pos.dim() == 4 else 1
        B = G * R
        z, _, box, q, _, dev = self._capture_inputs("capture_remd", "molecular dynamics needs", z, pos, None, box, q, B, K)
        if box is not None and tuple(box.shape) != (3, 3):
            raise ValueError(f"capture_remd: box must be one shared [3,3] box, got {tuple(box.shape)}")
        if q is not None:
            q = q.reshape(-1)
            if q.numel() != G:
                raise ValueError(f"capture_remd: q must have one entry per ladder ({G}), got {q.numel()}")
            q = torch.repeat_interleave(q, R).contiguous()
        m_all = masses.detach().to(device=dev, dtype=torch.float64).reshape(-1).repeat(B)
        if vel is None:  # Maxwell-Boltzmann at each slot's kT: sqrt(kT force_scale / m) per component, host generator
            gen = torch.Generator().manual_seed(int(thermostat.get("seed", 0)) & (2 ** 63 - 1))
            sd = torch.sqrt(kT[:, None] * float(force_scale) / masses.detach().cpu().to(torch.float64).reshape(1, n))  # [R,n]; m = inf: 0
            vel = (torch.randn((G, R, n, 3), generator=gen, dtype=torch.float64) * sd[None, :, :, None]).to(torch.float32).to(dev)
        return DeviceREMD(self, z.repeat(B).contiguous(), pos.reshape(-1, 3), vel.reshape(-1, 3), m_all, dt, kT, X, G, box, q, K, force_scale,
                          dict(thermostat), warmup)

    def capture_minimize(self, z: Tensor, pos: Tensor, batch: Optional[Tensor] = None, box: Optional[Tensor] = None,
                         q: Optional[Tensor] = None, num_systems: Optional[int] = None, steps_per_replay: int = 10,
                         fmax: float = 0.05, fire: Optional[dict] = None, fixed: Optional[Tensor] = None, warmup: int = 3,
                         lbfgs: Optional[dict] = None, atom_weights=None, halo_exchange=None, cell: Optional[dict] = None):
        """Capture ``steps_per_replay`` steps of a FIRE geometry minimisation into ONE HIP graph (needs ``static_shapes=True``): per
        step the per-atom update, neighbour list + energy + forces, the per-molecule sums and the controller, all as HIP kernels
        between the evaluations (``tmdnet_min_advance``) - no host work between steps.  FIRE as ASE ships it, unit masses, one
        controller per molecule: every molecule of a batch has its own time step and stops moving at the step where its largest
        atomic force norm falls below ``fmax``.  ``fire`` overrides ASE's defaults ``dict(dt=0.1, dt_max=1.0, n_min=5, f_inc=1.1,
        f_dec=0.5, alpha=0.1, f_alpha=0.99, max_step=0.2)``; ``fixed`` [N] marks atoms that never move.  The box is fixed unless
        ``cell`` is given.  Works for every architecture ``capture`` serves.  Returns a ``torchmdnet_amd.minimize.DeviceMinimizer``:
        ``opt(n)`` replays n times; ``opt.pos / forces``, ``opt.epot / fmax`` [K,B], ``opt.converged_at / step_size`` [B],
        ``opt.check()``, ``opt.reset(pos)``, ``opt.run(max_steps, check_every)``.  Inputs are staged and kept alive as in
        ``capture``.  ``atom_weights`` / ``halo_exchange`` are accepted only to be refused.
        ``cell=dict(mask=None, hydrostatic=False, constant_volume=False, pressure=0.0, cell_factor=None)`` relaxes the box together
        with the atoms inside the graph (``tmdnet_min_advance_cell``): ASE's ``UnitCellFilter`` scheme, one deformation gradient per
        molecule driven by the virial of every step towards ``pressure`` (E / length^3).  ``mask`` [3,3] of 0 / 1, symmetric, selects
        the entries of the cell force that act (None: all); ``hydrostatic`` keeps the shape, ``constant_volume`` the volume;
        ``cell_factor`` (None: the molecule's number of atoms) weighs the cell rows against the atoms.  Needs a box per molecule ([3,3]
        for one molecule, [B,3,3] otherwise) and an architecture with a virial (not TensorNet2).  Then ``opt.box`` (the caller's tensor
        when it needed no conversion), ``opt.deform`` [B,3,3], ``opt.stress`` [K,B,3,3] = -W_s / V, ``opt.volume`` [K,B],
        ``opt.reset(pos=, box=)``; ``opt.fmax`` includes the cell rows.  A fixed atom follows the cell affinely.  ``cell=None`` is the
        fixed-box path, unchanged.
        ``lbfgs=dict(memory=100, alpha=70.0, max_step=0.2, damping=1.0)`` (``{}``: these defaults, ASE's) minimises with L-BFGS instead
        of FIRE (``tmdnet_lbfgs_advance``): ASE's ``LBFGS`` without line search, one history per molecule, the step of every atom
        clamped to ``max_step``; a pair enters the history only when s.y > 0.  The workspace holds 24 (memory + 1) bytes per atom and
        24 (memory + 1)^2 per molecule: a batch of thousands of small molecules picks a smaller ``memory``.  Not together with ``fire``
        (ValueError) or ``cell`` (NotImplementedError).  Returns a ``torchmdnet_amd.lbfgs.DeviceLBFGS``: ``opt(n)``, ``opt.run``,
        ``opt.pos / forces / direction``, ``opt.epot / fmax / scale / accepted`` [K,B], ``opt.pairs / converged_at`` [B],
        ``opt.check()``, ``opt.reset(pos=)``.  ``lbfgs=None`` is the FIRE path, unchanged."""
        from torchmdnet_amd.minimize import DeviceMinimizer, parse_cell, parse_fire

        if not float(fmax) > 0:
            raise ValueError(f"fmax must be positive, got {fmax}")
        if lbfgs is not None:  # refused before anything is staged
            from torchmdnet_amd.lbfgs import DeviceLBFGS, parse_lbfgs

            parse_lbfgs(lbfgs)
            if fire is not None:
                raise ValueError("capture_minimize: lbfgs and fire exclude each other (one optimiser drives the minimisation)")
            if cell is not None:
                raise NotImplementedError("capture_minimize(lbfgs=...) has no HIP path with cell=...: the cell rows are not part of "
                                          "the L-BFGS history; relax the cell with FIRE")
        parse_fire(fire)
        if fixed is not None and fixed.numel() != z.shape[0]:
            raise ValueError(f"fixed must have one entry per atom ({z.shape[0]}), got {fixed.numel()}")
        z, batch, box, q, n_mol, _ = self._capture_inputs("capture_minimize", "a minimisation needs", z, pos, batch, box, q, num_systems,
                                                          steps_per_replay, atom_weights, halo_exchange, box_moves=cell is not None)
        if lbfgs is not None:
            return DeviceLBFGS(self, z, pos, batch, box, q, n_mol, steps_per_replay, fmax, lbfgs, fixed, warmup)
        if cell is not None:  # refused before anything is allocated or captured
            parse_cell(cell)
            self._refuse_virial()
            if box is None:
                raise ValueError("capture_minimize(cell=...) needs a box: the cell relaxation moves it")
            if box.dim() == 2 and n_mol > 1:
                raise NotImplementedError("capture_minimize(cell=...) relaxes one cell per molecule: give every molecule its own box "
                                          f"[{n_mol},3,3], not one shared [3,3] box")
            if bool((torch.linalg.det(box.detach().to(torch.float64)) == 0).any()):
                raise ValueError("capture_minimize(cell=...): a box has no volume")
        return DeviceMinimizer(self, z, pos, batch, box, q, n_mol, steps_per_replay, fmax, fire, fixed, warmup, cell)

    def capture_neb(self, z: Tensor, images: Tensor, box: Optional[Tensor] = None, q: Optional[Tensor] = None,
                    steps_per_replay: int = 10, fmax: float = 0.05, spring: float = 0.1, climb: bool = False,
                    fire: Optional[dict] = None, fixed: Optional[Tensor] = None, warmup: int = 3):
        """Capture ``steps_per_replay`` steps of a nudged-elastic-band path optimisation into ONE HIP graph (needs
        ``static_shapes=True``): a minimum-energy path between two minima and, with ``climb=True``, its saddle point.  ``z`` [n];
        ``images`` [M,n,3] (one band) or [G,M,n,3] (G bands), M >= 3, an unwrapped path whose first and last image never move
        (``torchmdnet_amd.neb.interpolate`` makes a linear one).  The G M images are evaluated as one batch; per step the per-atom
        update, neighbour list + energies + forces, the improved tangent of every interior image, the band force F_neb =
        F - (F.t)t + spring (|d+| - |d-|) t (the climber: F - 2 (F.t)t) and FIRE with one controller per band, all as HIP kernels
        between the evaluations (``tmdnet_neb_advance``) - no host work between steps.  A band stops moving at the step where its
        largest atomic |F_neb| falls below ``fmax``.  ``spring`` in E / length^2; ``fire`` as for ``capture_minimize``; ``fixed`` [n]
        marks atoms that never move in any image; a [3,3] ``box`` is shared by all images; ``q``, if given, is one value per band.
        Works for every architecture ``capture_minimize`` serves.  Returns a ``torchmdnet_amd.neb.DeviceNEB``: ``neb(n)`` replays n
        times; ``neb.images / forces`` [G,M,n,3], ``neb.epot`` [K,G,M], ``neb.fmax / climber`` [K,G], ``neb.converged_at /
        step_size`` [G], ``neb.barrier()``, ``neb.check()``, ``neb.reset(images=None, climb=None)``, ``neb.run(max_steps,
        check_every)``.  The same graph serves the plain and the climbing phase: ``neb.reset(climb=True)``."""
        from torchmdnet_amd.minimize import parse_fire
        from torchmdnet_amd.neb import DeviceNEB, parse_neb

        if not float(fmax) > 0:
            raise ValueError(f"fmax must be positive, got {fmax}")
        parse_fire(fire)
        parse_neb(dict(spring=spring, climb=climb))
        if z.dim() != 1:
            raise ValueError(f"z must be [n], the atoms of ONE image, got {tuple(z.shape)}")
        n = int(z.shape[0])
        if images.dim() not in (3, 4) or tuple(images.shape[-2:]) != (n, 3):
            raise ValueError(f"images must be [M,{n},3] or [G,M,{n},3] for {n} atoms, got {tuple(images.shape)}")
        if images.shape[-3] < 3:
            raise ValueError(f"a band needs at least 3 images, got {images.shape[-3]}")
        if images.dim() == 4 and images.shape[0] < 1:
            raise ValueError("images holds no band")
        n_bands = 1 if images.dim() == 3 else int(images.shape[0])
        if fixed is not None and fixed.numel() != n:
            raise ValueError(f"fixed must have one entry per atom of an image ({n}), got {fixed.numel()}")
        if q is not None and q.numel() != n_bands:
            raise ValueError(f"q must have one entry per band ({n_bands}), got {q.numel()}")
        z, _, box, q, _, _ = self._capture_inputs("capture_neb", "a band needs", z, images, None, box, q,
                                                  n_bands * int(images.shape[-3]), steps_per_replay, coords="the images")
        if box is not None and box.dim() != 2:
            raise ValueError(f"capture_neb takes one [3,3] box shared by all images, got {tuple(box.shape)}")
        q = None if q is None else q.reshape(-1)
        images = images if images.dim() == 4 else images[None]
        return DeviceNEB(self, z, images, box, q, steps_per_replay, fmax, spring, climb, fire, fixed, warmup)

    def capture_dimer(self, z: Tensor, pos: Tensor, mode: Optional[Tensor] = None, box: Optional[Tensor] = None,
                      q: Optional[Tensor] = None, steps_per_replay: int = 10, fmax: float = 0.05, delta: float = 0.01,
                      translate: bool = True, seed: int = 0, fire: Optional[dict] = None, fixed: Optional[Tensor] = None,
                      warmup: int = 3):
        """Capture ``steps_per_replay`` steps of a dimer (minimum-mode-following) saddle search into ONE HIP graph (needs
        ``static_shapes=True``): a first-order saddle point from ONE known state.  ``z`` [n]; ``pos`` [n,3] (one dimer) or [G,n,3]
        (G dimers of the same atoms); ``mode`` [n,3] or [G,n,3], the start axis (None: a seeded normal draw per dimer, ``seed``); the
        axis and a seeded partner direction at a right angle are orthonormalised in fp64 on the host.  Every step evaluates the
        midpoint R0, R0 + delta N and R0 + delta M of all dimers as one batch of 3 G molecules; the curvatures, the rotation of the
        axis towards the lowest mode, the force with its component along the axis inverted (F0 - 2 (F0.N) N where the curvature C is
        negative, -(F0.N) N where it is not) and FIRE with one controller per dimer run as HIP kernels between the evaluations
        (``tmdnet_dimer_advance``) - no host work between steps.  A dimer stops moving at the step where its largest atomic |F_eff|
        falls below ``fmax`` with C < 0.  ``delta`` in length units (forward differences: 0.01, the default of
        ``hessian(method="central")``); ``translate=False`` keeps the midpoint and only refines the mode and C; ``fire`` as for
        ``capture_minimize``; ``fixed`` [n] marks atoms that never move and carry no mode; a [3,3] ``box`` is shared by all images;
        ``q``, if given, is one value per dimer.  Works for every architecture ``capture_minimize`` serves.  Returns a
        ``torchmdnet_amd.dimer.DeviceDimer``: ``dimer(n)`` replays n times; ``dimer.pos / mode / forces / effective_forces``
        [G,n,3], ``dimer.epot / curvature / fmax / residual`` [K,G], ``dimer.converged_at / step_size`` [G], ``dimer.check()``,
        ``dimer.reset(pos=None, mode=None, translate=None)``, ``dimer.run(max_steps, check_every)``."""
        from torchmdnet_amd.dimer import DeviceDimer, orthonormal_pair
        from torchmdnet_amd.minimize import parse_fire

        if not float(fmax) > 0:
            raise ValueError(f"fmax must be positive, got {fmax}")
        if not (float(delta) > 0 and float(delta) < float("inf")):
            raise ValueError(f"delta must be positive and finite, got {delta}")
        parse_fire(fire)
        if z.dim() != 1:
            raise ValueError(f"z must be [n], the atoms of ONE dimer image, got {tuple(z.shape)}")
        n = int(z.shape[0])
        if pos.dim() not in (2, 3) or tuple(pos.shape[-2:]) != (n, 3):
            raise ValueError(f"pos must be [{n},3] or [G,{n},3] for {n} atoms, got {tuple(pos.shape)}")
        if pos.dim() == 3 and pos.shape[0] < 1:
            raise ValueError("pos holds no dimer")
        n_dimers = 1 if pos.dim() == 2 else int(pos.shape[0])
        if mode is not None and tuple(mode.shape) not in ((n, 3), (n_dimers, n, 3)):
            raise ValueError(f"mode must be [{n},3] or [{n_dimers},{n},3], got {tuple(mode.shape)}")
        if fixed is not None and fixed.numel() != n:
            raise ValueError(f"fixed must have one entry per atom of an image ({n}), got {fixed.numel()}")
        if q is not None and q.numel() != n_dimers:
            raise ValueError(f"q must have one entry per dimer ({n_dimers}), got {q.numel()}")
        N, M = orthonormal_pair(mode, n_dimers, n, fixed, seed)  # (raises for a mode that is zero on the free atoms)
        z, _, box, q, _, _ = self._capture_inputs("capture_dimer", "a dimer needs", z, pos, None, box, q, 3 * n_dimers, steps_per_replay)
        if box is not None and box.dim() != 2:
            raise ValueError(f"capture_dimer takes one [3,3] box shared by all images, got {tuple(box.shape)}")
        q = None if q is None else q.reshape(-1)
        pos = pos if pos.dim() == 3 else pos[None]
        return DeviceDimer(self, z, pos, N.to(pos.device), M.to(pos.device), box, q, steps_per_replay, fmax, delta, translate, fire, fixed,
                           warmup)

    def capture_irc(self, z: Tensor, pos: Tensor, mode: Tensor, masses: Tensor, dt: float, direction: str = "both",
                    box: Optional[Tensor] = None, q: Optional[Tensor] = None, steps_per_replay: int = 10, force_scale: float = 1.0,
                    fmax: float = 0.05, v0: float = 0.02, error: float = 1.5e-3, initial_step: float = 0.05,
                    dt_min: Optional[float] = None, dt_max: Optional[float] = None, record: Optional[dict] = dict(every=1, capacity=512),
                    fixed: Optional[Tensor] = None, warmup: int = 3):
        """Capture ``steps_per_replay`` steps of an intrinsic-reaction-coordinate (IRC) follower into ONE HIP graph (needs
        ``static_shapes=True``): the path of steepest descent in mass-weighted coordinates from a saddle point, which shows the two
        minima the saddle connects and the energy profile E(s) between them.  ``z`` [n]; ``pos`` [n,3] (one saddle) or [G,n,3] (G
        saddles of the same atoms); ``mode`` [n,3] or [G,n,3], a Cartesian direction along the transition vector (``dimer.mode``, or a
        column of ``vib.displacements()`` reshaped), normalised in fp64 on the host; ``masses`` [n]; ``dt`` the first time step.
        ``direction``: "both" (every saddle runs forward, along ``mode``, and backward), "forward" or "backward".  The damped
        velocity Verlet path follower (Hratchian and Schlegel, J. Phys. Chem. A 106, 165, 2002): a trajectory with
        a = ``force_scale`` F / m from x_TS +- ``initial_step`` u whose speed is put back to ``v0`` after every step, so that it
        moves along F / m; each path chooses its own time step so that the estimated error of a step stays near ``error`` (a length),
        between ``dt_min`` and ``dt_max`` (None: dt / 16 and 16 dt).  The paths of all saddles are evaluated as one batch and the
        integrator, the controllers and the path record run as HIP kernels between the evaluations (``tmdnet_irc_advance``) - no host
        work between steps.  A path finishes at the step where its largest atomic |F| falls below ``fmax`` (reason 1) or where it
        turns uphill (reason 2: the minimum lies within one step behind it; ``capture_minimize`` from ``irc.pos`` relaxes it).  The
        defaults of ``v0`` and ``error`` are the paper's 0.04 bohr/fs and 0.003 bohr in Angstrom and fs.  ``record`` =
        dict(every=S, capacity=C) keeps every S-th point of a path, the start image and its last point on the device, at most C per
        path (``irc.truncated`` tells when more were taken).  ``fixed`` [n] marks atoms that never move; a [3,3] ``box`` is shared by
        all paths; ``q``, if given, is one value per saddle.  Works for every architecture ``capture_minimize`` serves.  Returns a
        ``torchmdnet_amd.irc.DeviceIRC``: ``irc(n)`` replays n times; ``irc.pos / vel / forces`` [G,D,n,3], ``irc.epot / fmax /
        arc / dt / power`` [K,G,D], ``irc.converged_at / reason / step_size / arc_length / n_recorded`` [G,D], ``irc.check()``,
        ``irc.reset(pos=None, mode=None)``, ``irc.run(max_steps, check_every)``, ``irc.path(g)`` -> dict(s, energy, pos)."""
        from torchmdnet_amd.irc import _DIRECTIONS, DeviceIRC, unit_direction

        if direction not in _DIRECTIONS:
            raise ValueError(f"direction must be one of {sorted(_DIRECTIONS)}, got {direction!r}")
        for name, value in (("fmax", fmax), ("v0", v0), ("error", error), ("initial_step", initial_step), ("dt", dt), ("force_scale", force_scale)):
            if not (float(value) > 0 and float(value) < float("inf")):
                raise ValueError(f"{name} must be positive and finite, got {value}")
        dt_min = float(dt) / 16.0 if dt_min is None else float(dt_min)
        dt_max = float(dt) * 16.0 if dt_max is None else float(dt_max)
        if not (dt_min > 0 and dt_max < float("inf")) or dt_min > dt_max:
            raise ValueError(f"dt_min and dt_max must be positive, finite and ordered, got {dt_min} and {dt_max}")
        record = dict(every=1, capacity=512) if record is None else dict(record)
        every, capacity = int(record.pop("every", 1)), int(record.pop("capacity", 512))
        if record:
            raise ValueError(f"record takes every and capacity, got also {sorted(record)}")
        if every < 1 or capacity < 1:
            raise ValueError(f"record needs every >= 1 and capacity >= 1, got every={every}, capacity={capacity}")
        if z.dim() != 1:
            raise ValueError(f"z must be [n], the atoms of ONE saddle, got {tuple(z.shape)}")
        n = int(z.shape[0])
        if pos.dim() not in (2, 3) or tuple(pos.shape[-2:]) != (n, 3):
            raise ValueError(f"pos must be [{n},3] or [G,{n},3] for {n} atoms, got {tuple(pos.shape)}")
        if pos.dim() == 3 and pos.shape[0] < 1:
            raise ValueError("pos holds no saddle")
        n_saddles = 1 if pos.dim() == 2 else int(pos.shape[0])
        if tuple(mode.shape) not in ((n, 3), (n_saddles, n, 3)):
            raise ValueError(f"mode must be [{n},3] or [{n_saddles},{n},3], got {tuple(mode.shape)}")
        if masses.numel() != n:
            raise ValueError(f"masses must have one entry per atom of a saddle ({n}), got {masses.numel()}")
        if not bool((masses.detach() > 0).all()):
            raise ValueError("masses must be positive")
        if fixed is not None and fixed.numel() != n:
            raise ValueError(f"fixed must have one entry per atom of a saddle ({n}), got {fixed.numel()}")
        if q is not None and q.numel() != n_saddles:
            raise ValueError(f"q must have one entry per saddle ({n_saddles}), got {q.numel()}")
        still = torch.isinf(masses.detach().cpu().reshape(-1))
        if fixed is not None:
            still = still | (fixed.detach().cpu().reshape(-1) != 0)
        u = unit_direction(mode, n_saddles, n, still)  # (raises for a mode that is zero on the atoms that move)
        signs = _DIRECTIONS[direction]
        z, _, box, q, _, _ = self._capture_inputs("capture_irc", "a path needs", z, pos, None, box, q, len(signs) * n_saddles, steps_per_replay)
        if box is not None and box.dim() != 2:
            raise ValueError(f"capture_irc takes one [3,3] box shared by all paths, got {tuple(box.shape)}")
        q = None if q is None else q.reshape(-1)
        pos = pos if pos.dim() == 3 else pos[None]
        return DeviceIRC(self, z, pos, u.to(pos.device), masses, dt, signs, box, q, steps_per_replay, force_scale, fmax, v0, error, initial_step,
                         dt_min, dt_max, every, capacity, fixed, warmup)

    def capture_scan(self, z: Tensor, pos: Tensor, cvs, targets: Tensor, box: Optional[Tensor] = None, q: Optional[Tensor] = None,
                     steps_per_replay: int = 10, fmax: float = 0.05, drive=None, tol: float = 1e-8, max_iter: int = 16,
                     fire: Optional[dict] = None, fixed: Optional[Tensor] = None, warmup: int = 3):
        """Capture ``steps_per_replay`` steps of a relaxed coordinate scan into ONE HIP graph (needs ``static_shapes=True``): the
        molecule minimised with chosen internal coordinates held at exact values - a torsion or bond profile, a first guess of a
        reaction path.  ``z`` [n]; ``pos`` [n,3] (one start geometry for every point) or [G,n,3]; ``cvs`` = [("distance", i, j),
        ("angle", i, j, k), ("torsion", i, j, k, l), ...], 1 to 4 collective variables as ``capture_md_biased`` takes them, indices
        within the molecule, on the unwrapped positions without minimum image; ``targets`` [G,D], the final values of the D CVs at
        each of the G points (``torchmdnet_amd.scan.grid(start, stop, n)`` makes a scan along one CV).  The G points are evaluated as
        one batch.  Per step the force and FIRE's velocity are projected onto the tangent space of the constraints with Lagrange
        multipliers from the D x D Gram matrix of the CV gradients, FIRE with one controller per point moves the atoms, every target
        moves by at most ``drive`` (per CV; None: 0.1 rad for an angle or torsion, 0.05 length units for a distance) from the CV of
        the start geometry towards its final value - a torsion the short way round - and up to ``max_iter`` Gauss-Newton corrections
        put the CV atoms back on the constraint surface to within ``tol``: HIP kernels between the evaluations
        (``tmdnet_scan_advance``), no host work between steps.  A point stops moving at the step where its largest atomic |F_perp|
        falls below ``fmax`` with its targets at their final values.  ``fire`` as for ``capture_minimize``; ``fixed`` [n] marks atoms
        that never move (a CV may contain some, not only, fixed atoms); a [3,3] ``box`` is shared by all points; ``q``, if given, is
        one value per point.  Works for every architecture ``capture_minimize`` serves.  Returns a
        ``torchmdnet_amd.scan.DeviceScan``: ``scan(n)`` replays n times; ``scan.pos / forces / projected_forces`` [G,n,3],
        ``scan.epot / fmax`` [K,G], ``scan.cv / target / multiplier`` [K,G,D] (dE/dt = -multiplier at a constrained minimum),
        ``scan.converged_at / step_size`` [G], ``scan.check()``, ``scan.reset(pos=, targets=)``, ``scan.run(max_steps,
        check_every)``, ``scan.profile()`` -> dict(target, cv, energy, multiplier, converged)."""
        from torchmdnet_amd.minimize import parse_fire
        from torchmdnet_amd.scan import DeviceScan, parse_cvs, parse_drive

        if not float(fmax) > 0:
            raise ValueError(f"fmax must be positive, got {fmax}")
        if not (float(tol) > 0 and float(tol) < float("inf")):
            raise ValueError(f"tol must be positive and finite, got {tol}")
        if int(max_iter) < 1:
            raise ValueError(f"max_iter must be at least 1, got {max_iter}")
        parse_fire(fire)
        if z.dim() != 1:
            raise ValueError(f"z must be [n], the atoms of ONE point, got {tuple(z.shape)}")
        n = int(z.shape[0])
        if pos.dim() not in (2, 3) or tuple(pos.shape[-2:]) != (n, 3):
            raise ValueError(f"pos must be [{n},3] or [G,{n},3] for {n} atoms, got {tuple(pos.shape)}")
        if fixed is not None and fixed.numel() != n:
            raise ValueError(f"fixed must have one entry per atom of a point ({n}), got {fixed.numel()}")
        kinds, atoms, distinct = parse_cvs(cvs, n, fixed)
        drive = parse_drive(drive, kinds)
        if targets.dim() != 2 or targets.shape[0] < 1 or targets.shape[1] != len(kinds):
            raise ValueError(f"targets must be [G,{len(kinds)}], one row per point and one column per collective variable, got "
                             f"{tuple(targets.shape)}")
        if not bool(torch.isfinite(targets).all()):
            raise ValueError("targets must be finite")
        n_points = int(targets.shape[0])
        if pos.dim() == 3 and pos.shape[0] != n_points:
            raise ValueError(f"pos holds {pos.shape[0]} start geometries for {n_points} rows of targets")
        if q is not None and q.numel() != n_points:
            raise ValueError(f"q must have one entry per point ({n_points}), got {q.numel()}")
        if box is not None and box.dim() != 2:  # (before anything is staged; the model's own box is looked at below)
            raise ValueError(f"capture_scan takes one [3,3] box shared by all points, got {tuple(box.shape)}")
        pos = (pos if pos.dim() == 3 else pos[None].expand(n_points, n, 3)).contiguous()
        z, _, box, q, _, _ = self._capture_inputs("capture_scan", "a scan needs", z, pos, None, box, q, n_points, steps_per_replay)
        if box is not None and box.dim() != 2:
            raise ValueError(f"capture_scan takes one [3,3] box shared by all points, got {tuple(box.shape)}")
        q = None if q is None else q.reshape(-1)
        return DeviceScan(self, z, pos, kinds, atoms, distinct, targets, box, q, steps_per_replay, fmax, drive, tol, max_iter, fire, fixed,
                          warmup)

    def capture_minima_hopping(self, z: Tensor, pos: Tensor, masses: Tensor, dt: float, batch: Optional[Tensor] = None,
                               box: Optional[Tensor] = None, q: Optional[Tensor] = None, num_systems: Optional[int] = None,
                               steps_per_replay: int = 10, force_scale: float = 9.648533e-3, kT0: float = 0.05, ediff0: float = 0.05,
                               beta1: float = 1.1, beta2: float = 1.1, beta3: float = 1 / 1.1, alpha1: float = 0.98,
                               alpha2: float = 1 / 0.98, mdmin: int = 2, md_steps: int = 400, opt_steps: int = 2000, fmax: float = 0.05,
                               rmsd_tol: float = 0.1, energy_tol: float = 1e-3, capacity: int = 32, align: Optional[str] = None,
                               seed: int = 0, fire: Optional[dict] = None, fixed: Optional[Tensor] = None, warmup: int = 3,
                               atom_weights=None, halo_exchange=None):
        """Capture ``steps_per_replay`` steps of a minima-hopping conformer search into ONE HIP graph (needs ``static_shapes=True``):
        Goedecker, J. Chem. Phys. 120, 9911 (2004), parameters named as in ASE's ``MinimaHopping``.  The B molecules of the batch
        are B independent walkers (the batch may be ragged; copies of one molecule give a parallel search of it).  Each walker
        leaves its minimum by an NVE run with velocities drawn at ``kT`` - momentum and, with ``align="rotation"``, angular momentum
        removed on the device - until the energy along the run has passed ``mdmin`` minima or ``md_steps`` steps, quenches with FIRE
        to ``fmax`` (at most ``opt_steps`` steps), and compares the minimum it finds with the one it left and with a ring of
        ``capacity`` (1..64) recorded minima: the same geometry (rmsd < ``rmsd_tol`` and |dE| < ``energy_tol``) as the one it left
        scales kT by ``beta1``, a known one by ``beta2``, a new one by ``beta3``; a new minimum is accepted when it lies less than
        ``ediff`` above the current one (``ediff *= alpha1``) and rejected otherwise (``ediff *= alpha2``).  ``align`` chooses the
        rmsd: ``"rotation"`` (Horn's quaternion method; the default without a box and without fixed atoms), ``"translation"`` (the
        default with a box) or ``"none"`` (the default with fixed atoms).  Every step is one evaluation shared by walkers in
        different phases plus three launches (``tmdnet_hop_advance``) - no host work between steps.  Units, ``force_scale``,
        ``masses`` and ``dt`` are ``capture_md``'s; ``fixed`` [N] marks atoms of infinite mass and zero velocity; ``fire`` is
        ``capture_minimize``'s; ``kT0`` and ``ediff0`` in the unit of the energy.  Works for every architecture ``capture_md``
        serves.  ``atom_weights`` / ``halo_exchange`` are accepted only to be refused.  Returns a ``torchmdnet_amd.hop.DeviceHop``:
        ``hop(n)``, ``hop.run(hops, max_steps)``, ``hop.check()``, ``hop.reset(pos=, kT=, ediff=, history=)``, ``hop.pos / vel /
        forces``, ``hop.phase / kT / ediff``, ``hop.minimum_pos / minimum_energy / best_pos / best_energy``, ``hop.n_hops / n_same /
        n_known / n_new / n_accepted / n_unconverged``, the logs ``hop.epot / fmax / ekin / phase_log / outcome`` [K,B] and
        ``hop.minima(b)``."""
        from torchmdnet_amd.hop import DeviceHop, parse_hop

        N = int(z.shape[0])
        if masses.numel() != N:
            raise ValueError(f"masses must have one entry per atom ({N}), got {masses.numel()}")
        if fixed is not None and fixed.numel() != N:
            raise ValueError(f"fixed must have one entry per atom ({N}), got {fixed.numel()}")
        if not (float(force_scale) > 0):
            raise ValueError(f"force_scale must be positive, got {force_scale}")
        m = masses.detach().to(torch.float64)
        if not bool(((m > 0) & ~torch.isnan(m)).all()):
            raise ValueError("masses must be positive (infinite: a fixed atom)")
        has_fixed = (fixed is not None and bool((fixed != 0).any())) or bool(torch.isinf(m).any())
        has_box = box is not None or bool(self.representation_model.distance.use_periodic)
        params = parse_hop(dt, kT0, ediff0, fire, align, has_box, has_fixed, beta1=beta1, beta2=beta2, beta3=beta3, alpha1=alpha1,
                           alpha2=alpha2, mdmin=mdmin, md_steps=md_steps, opt_steps=opt_steps, fmax=fmax, rmsd_tol=rmsd_tol,
                           energy_tol=energy_tol, capacity=capacity, seed=seed)
        z, batch, box, q, n_mol, _ = self._capture_inputs("capture_minima_hopping", "minima hopping needs", z, pos, batch, box, q,
                                                          num_systems, steps_per_replay, atom_weights, halo_exchange)
        return DeviceHop(self, z, pos, masses, batch, box, q, n_mol, steps_per_replay, force_scale, params, fixed, warmup)

    def hessian(self, z: Tensor, pos: Tensor, batch: Optional[Tensor] = None, box: Optional[Tensor] = None, q: Optional[Tensor] = None,
                method: str = "analytic", delta: float = 0.01, fixed: Optional[Tensor] = None, replicas: Optional[int] = None,
                max_workspace_bytes: int = 8 << 30, atom_weights=None):
        """The Hessian d^2 E_b / d x d x of every molecule of a batch, assembled on the device: ``(H, info)`` with ``H`` [B,D,D] fp32
        (padded, row-major; molecule b fills its leading D_b = 3 nfree_b rows and columns, coordinate i = component i % 3 of its free
        atom i / 3) and ``info`` a dict (``dims``, ``replicas``, ``passes``, ``engine_calls``, ``graph_builds``, ``free_idx``,
        ``fstart``, ...).  R replicas of the batch, each carrying one coordinate of every molecule, give R columns of every molecule
        per pass (``tmdnet_vib_seed`` / ``tmdnet_vib_gather``).  ``method="analytic"``: one second-order pass per R columns
        (``tmdnet_loss_param_grads`` with a unit seed; the neighbour graph of the replicated batch is built once).
        ``method="central"``: two ``energy_and_forces`` evaluations per R columns at ``pos +- delta``; the quotient divides by the
        actual difference of the rounded positions.  ``batch`` must be non-decreasing; ``fixed`` [N] removes atoms from the Hessian
        (a partial Hessian); ``replicas=None`` picks the largest R <= D whose workspace fits ``max_workspace_bytes``.  ``atom_weights``
        is served by the central route only.  Works for TensorNet, the Equivariant Transformer and TensorNet2 with the scalar head."""
        from torchmdnet_amd.vibrations import compute_hessian

        return compute_hessian(self, z, pos, batch, box, q, method, delta, fixed, replicas, max_workspace_bytes, atom_weights)

    def vibrations(self, z: Tensor, pos: Tensor, batch: Optional[Tensor] = None, box: Optional[Tensor] = None, q: Optional[Tensor] = None,
                   masses: Optional[Tensor] = None, project: bool = True, force_scale: float = 9.648533e-3, **hessian_kw):
        """Normal-mode analysis at ``pos``: ``hessian(...)``, then on the device and in fp64 the symmetrisation, the mass weighting and
        the projection of translations and rotations (``tmdnet_vib_finish``: translations only with a box, nothing for a molecule
        with a fixed atom or with ``project=False``), then ``torch.linalg.eigh`` per molecule on the host.  ``masses`` [N] (default:
        ``torchmdnet_amd.atomic_masses.atomic_masses[z]``); ``force_scale`` converts E / (length^2 mass) into the squared angular
        frequency of ``omega2`` (default: eV, Angstrom, amu -> fs^-2); ``hessian_kw``: ``method``, ``delta``, ``fixed``,
        ``replicas``, ``max_workspace_bytes``.  Returns a ``torchmdnet_amd.vibrations.Vibrations``: ``eigenvalues``, ``modes``,
        ``omega2``, ``wavenumbers()``, ``n_negative()``, ``zero_point_energy()``, ``n_projected``, ``asymmetry``, ``drift``,
        ``hmax``, ``hessian``."""
        from torchmdnet_amd.vibrations import compute_vibrations

        return compute_vibrations(self, z, pos, batch, box, q, masses, project, force_scale, **hessian_kw)

    def debug_tensor(self, name: str, shape) -> Tensor:
        L = _C.lib()
        st = self._engine
        dev = st.fwd_ws.device
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        rc = L.tmdnet_debug_tensor(st.handle, _stream_ptr(dev), name.encode(), _ptr(out), out.numel())
        if rc != _C.OK:
            raise RuntimeError(L.tmdnet_last_error(st.handle).decode())
        return out

    def _forward_host_tensors(self, z, pos, batch, box, q, num_systems):
        """HOST tensors (the reference's default: `create_model(args)` and `torch.randn(...)` live on the CPU, tests/test_model.py):
        the inputs are staged to the current AMD GPU, the HIP engine computes there, and the outputs come back as host tensors on
        `pos.device` - the boundary "hands over host buffers" (DESIGN: PCIe-inclusive).  This is NOT a CPU path: without a GPU the
        call fails exactly as before.  The moves are autograd-visible (`Tensor.to`), so `energy.backward()` and `pos.grad` work on
        the caller's host tensors; a module whose parameters live on the host is uploaded to the engine from there."""
        dev = torch.device("cuda", torch.cuda.current_device())
        pdev = next(self.parameters()).device
        if pdev.type == "cuda":
            dev = pdev
        mv = lambda t: None if t is None else t.to(dev)
        y, f = self.forward(z.to(dev), pos.to(dev), mv(batch), mv(box), mv(q), None, None, num_systems)
        return y.to(pos.device), f.to(pos.device)

    # ---------------------------------------------------------------- reference-compatible forward
    def forward(self, z: Tensor, pos: Tensor, batch: Optional[Tensor] = None, box: Optional[Tensor] = None,
                q: Optional[Tensor] = None, s: Optional[Tensor] = None, extra_args: Optional[Dict[str, Tensor]] = None,
                num_systems: Optional[int] = None) -> Tuple[Tensor, Tensor]:
        assert z.dim() == 1 and z.dtype == torch.long
        batch = torch.zeros_like(z) if batch is None else batch
        if pos.dtype != torch.float32:
            raise NotImplementedError("torchmdnet_amd computes in fp32; cast positions to float32")
        if self.derivative:
            pos.requires_grad_(True)  # reference side effect (model.py:584-585)
        if pos.device.type == "cpu" and torch.cuda.is_available():  # without a GPU: _require_cuda below raises, as ever
            return self._forward_host_tensors(z, pos, batch, box, q, num_systems)
        if num_systems is not None:
            n_mol = int(num_systems)
        else:
            # reference OutputModel.reduce (output_modules.py:43-73): the molecule count is read from `batch` (a host sync)
            # except while the stream is being captured into a CUDA/HIP graph, where the value of the warm-up calls is used
            capturing = pos.is_cuda and torch.cuda.is_current_stream_capturing()
            if not capturing:
                self.output_model.dim_size = int(batch.max().item()) + 1 if z.numel() else 0
            else:
                assert self.output_model.dim_size > 0, "Warming up is needed before capturing the model into a CUDA graph"
            n_mol = self.output_model.dim_size
        rm = self.representation_model
        if box is None and rm.distance.use_periodic:
            box = rm.distance.box
        if box is not None and box.device != pos.device:
            box = box.to(pos.device)  # a host-resident module evaluated through _forward_host_tensors
        want_forces = bool(self.derivative or (pos.requires_grad and torch.is_grad_enabled()))
        _require_cuda(pos, "TorchMD_Net.forward")
        if self.parameter_gradients and torch.is_grad_enabled():
            if self._head_kind() != _C.HEAD_SCALAR:
                raise NotImplementedError(f"parameter_gradients with output_model {type(self.output_model).__name__} has no HIP path "
                                          "(the property heads evaluate values and forces only)")
            params = [p for p in self.parameters() if p.requires_grad]
            if want_forces:  # force matching: forces carry a (finite-difference) graph to the parameters as well
                energy, forces = _EnergyForceParamGrad.apply(self, z, pos, batch, box, q, n_mol, *params)
                return energy.view(-1, 1), (forces if self.derivative else torch.empty(0, device=pos.device))
            return _EnergyParamGrad.apply(self, z, pos, batch, box, q, n_mol, *params).view(-1, 1), torch.empty(0, device=pos.device)
        if self._engine.op_key is None:
            self._engine.op_key = ops.register_engine(self)
        # one registered torch op (fake + autograd registered, torchmdnet_amd/ops.py): torch.compile / torch.export trace
        # through it, and `energy.backward()` (ASE calculator, OpenMM wrapper: reference calculators.py:311-316) gets
        # d(sum_m g_m E_m)/d pos_i = -g_{batch_i} F_i from its registered backward
        energy, forces = torch.ops.tmdnet.energy_forces(z, pos, batch, box, q, self._engine.op_key, n_mol, want_forces)
        y = energy.view(-1, 3) if energy.dim() == 2 else energy.view(-1, 1)  # [B,1], or [B,3] for the vector output
        if self.derivative:
            return y, forces.detach()
        # an empty tensor keeps the reference's "always two tensors" contract (model.py:629-631)
        return y, torch.empty(0, device=y.device)


class Ensemble(torch.nn.ModuleList):
    """Average (and optionally std) of several models' predictions (reference model.py:634-680)."""

    def __init__(self, modules: List[nn.Module], return_std: bool = False):
        for module in modules:
            assert isinstance(module, TorchMD_Net)
        super().__init__(modules)
        self.return_std = return_std

    def forward(self, *args, **kwargs):
        ys, fs = [], []
        for model in self:
            y, f = model(*args, **kwargs)
            ys.append(y)
            fs.append(f)
        y, f = torch.stack(ys), torch.stack(fs)
        if self.return_std:
            return torch.mean(y, axis=0), torch.mean(f, axis=0), torch.std(y, axis=0), torch.std(f, axis=0)
        return torch.mean(y, axis=0), torch.mean(f, axis=0)

    # ---------------------------------------------------------------- the committee on the device (torchmdnet_amd/committee.py)
    def committee(self, z: Tensor, pos: Tensor, batch: Optional[Tensor] = None, box: Optional[Tensor] = None,
                  q: Optional[Tensor] = None, num_systems: Optional[int] = None, atom_weights=None, halo_exchange=None):
        """Every member's ``energy_and_forces`` on the current stream, one after the other (each with its own architecture, cutoff,
        priors and box), then ONE pass on the device (``tmdnet_committee_reduce``, two launches): -> the named result
        ``committee.CommitteeResult(energy [B], forces [N,3], energy_std [B], forces_std [N,3], deviation [N], max_deviation [B],
        max_atom [B] int64)``: mean and unbiased standard deviation over the members (fp64 sums in two passes, rounded once - unlike
        ``forward``'s fp32 ``torch.std``, which is kept as it is), ``deviation[i] = sqrt(sum_c forces_std[i,c]^2)`` (+inf when not
        finite), and per molecule its maximum and the smallest atom index that attains it (0 and -1 without atoms).  2 to 16 members
        on one device, scalar heads, no training models; ``atom_weights`` / ``halo_exchange`` are accepted only to be refused."""
        from torchmdnet_amd import committee

        return committee.committee(self, z, pos, batch, box, q, num_systems, atom_weights, halo_exchange)

    def capture(self, z: Tensor, pos: Tensor, batch: Optional[Tensor] = None, box: Optional[Tensor] = None,
                q: Optional[Tensor] = None, num_systems: Optional[int] = None, warmup: int = 3, atom_weights=None, halo_exchange=None):
        """``committee`` captured into ONE HIP graph (every member needs ``static_shapes=True``): the members in member order on the
        capturing stream, then the pass.  Returns ``replay(pos=None)`` -> the same named result in static buffers; ``replay.pos`` are
        the positions the graph reads (write them in place to skip the copy), ``replay.inputs`` the staged inputs per member,
        ``replay.graph`` the graph, ``replay.member_outputs`` the members' own static (E, F).  A parameter change or device move of
        any member after the capture makes the next replay raise."""
        from torchmdnet_amd import committee

        return committee.capture(self, z, pos, batch, box, q, num_systems, warmup, atom_weights, halo_exchange)

    def capture_md(self, z: Tensor, pos: Tensor, vel: Tensor, masses: Tensor, dt: float, batch: Optional[Tensor] = None,
                   box: Optional[Tensor] = None, q: Optional[Tensor] = None, num_systems: Optional[int] = None,
                   steps_per_replay: int = 10, force_scale: float = 1.0, thermostat: Optional[dict] = None, warmup: int = 3,
                   gate: Optional[dict] = None, atom_weights=None, halo_exchange=None, barostat=None, constraints=None, bias=None,
                   temperatures=None):
        """``TorchMD_Net.capture_md`` driven by the committee: ``steps_per_replay`` MD steps in one HIP graph, every step with the M
        members' evaluations, the committee pass and the integrator on the MEAN forces; ``epot`` is the mean energy.  Returns a
        ``torchmdnet_amd.committee.DeviceCommitteeMD``: ``DeviceMD``'s surface plus the logs ``energy_std / deviation /
        deviation_atom`` [K,B] and the gate's state.
        ``gate=dict(flag_above=None | float, stop_above=None | float)``, thresholds on the molecule's largest force deviation D_m in
        the unit of the forces, compared as ``not (D_m <= threshold)`` so that a NaN never passes as certain.  ``flag_above``: the
        first time a molecule exceeds it, ``flagged_at[m]`` becomes the step and the molecule's atoms are copied into
        ``flagged_pos`` (with ``flagged_dev / flagged_atom``); the trajectory goes on.  ``stop_above``: the step is completed with
        the committee mean, then the loop freezes (status 6): ``stopped`` -> (step, molecule, atom, value), ``check()`` does not
        raise, ``run(max_steps)`` replays until stopped, ``reset(pos, vel, step, flags="keep" | "clear")`` starts again.  An overflowed
        neighbour list in any member freezes the loop at the last completed step and ``check()`` raises the reference's error.
        In this version the thermostat is None or Langevin (``dict(friction=, kT=, seed=)``); a global thermostat, ``barostat``,
        ``constraints``, ``bias``, replica exchange (``temperatures``), ``atom_weights`` and ``halo_exchange`` are refused."""
        from torchmdnet_amd import committee

        return committee.capture_md(self, z, pos, vel, masses, dt, batch, box, q, num_systems, steps_per_replay, force_scale,
                                    thermostat, warmup, gate, atom_weights, halo_exchange, barostat, constraints, bias, temperatures)
