"""ctypes binding of libtmdnet_amd.so (include/tmdnet_amd.h).

There is NO CPU fallback: if the shared library is missing or a symbol is absent the import of the
compute path fails loudly.  The library itself needs a gfx950 device only when a compute entry
point is called; dlopen + symbol lookup work on a CPU-only host (used by the "not gpu" tests).
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libtmdnet_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "tmdnet_amd.h")

OK, ERR_INVALID, ERR_HIP, ERR_OVERFLOW, ERR_WORKSPACE, ERR_STATE = 0, 1, 2, 3, 4, 5
# output heads of tmdnet_set_output_head
HEAD_SCALAR, HEAD_DIPOLE_MOMENT, HEAD_SPATIAL_EXTENT, HEAD_VECTOR = 0, 1, 2, 3


class HParams(C.Structure):
    _fields_ = [
        ("hidden_channels", C.c_int32),
        ("num_layers", C.c_int32),
        ("num_rbf", C.c_int32),
        ("max_z", C.c_int32),
        ("max_num_neighbors", C.c_int32),
        ("group_o3", C.c_int32),
        ("head_hidden", C.c_int32),
        ("has_atomref", C.c_int32),
        ("cutoff_lower", C.c_float),
        ("cutoff_upper", C.c_float),
    ]


class EtHParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("hidden_channels", "num_layers", "num_rbf", "max_z", "max_num_neighbors", "num_heads",
                                         "neighbor_embedding", "vector_cutoff", "distance_influence", "has_atomref")] + \
               [("cutoff_lower", C.c_float), ("cutoff_upper", C.c_float)]


class Tn2HParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("hidden_channels", "num_layers", "num_rbf", "max_z", "max_num_neighbors", "group_o3",
                                         "head_hidden", "has_atomref", "q_dim")] + \
               [("cutoff_lower", C.c_float), ("cutoff_upper", C.c_float), ("coulomb_cutoff", C.c_float),
                ("coulomb_epsilon_solvent", C.c_float)]


class GemmExArgs(C.Structure):
    """tmdnet_gemm_ex_args (include/tmdnet_amd.h): the argument surface of tmdnet_debug_gemm_ex."""
    _fields_ = [
        ("A", C.c_void_p), ("W", C.c_void_p * 9), ("bias", C.c_void_p * 9), ("C", C.c_void_p), ("pre", C.c_void_p),
        ("aux", C.c_void_p), ("rowscale", C.c_void_p),
        ("lda", C.c_int64), ("ldw", C.c_int64), ("ldc", C.c_int64), ("ldpre", C.c_int64), ("ldaux", C.c_int64),
        ("a_off", C.c_int32 * 9), ("c_off", C.c_int32 * 9), ("pre_off", C.c_int32 * 9), ("aux_off", C.c_int32 * 9),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("groups", C.c_int32), ("flags", C.c_int32),
        ("m_dev", C.c_void_p), ("m_add", C.c_int32),
        ("Wsbg", C.c_void_p * 9),
    ]


class MessageArgs(C.Structure):
    """tmdnet_message_args (include/tmdnet_amd.h): one neighbour sweep on a caller-built graph, tmdnet_debug_message."""
    _fields_ = [(n, C.c_int32) for n in ("op", "kernel", "N", "F", "P", "small_mols", "o3", "balance", "accumulate")] + \
               [(n, C.c_void_p) for n in ("rowptr", "col", "epair", "esign", "counts", "w", "w2", "src", "src2", "q", "batch", "out",
                                          "out2", "slots")] + [("slot_stride", C.c_int64)]


class MessageFoldArgs(C.Structure):
    """tmdnet_message_fold_args (include/tmdnet_amd.h): the reverse tile sweep with the group-product adjoint in its prologue, or
    the sequence it replaces, tmdnet_debug_message_fold."""
    _fields_ = [(n, C.c_int32) for n in ("N", "F", "P", "o3", "folded")] + \
               [(n, C.c_void_p) for n in ("rowptr", "col", "epair", "esign", "counts", "w", "dw", "gCh", "Pn", "Mi", "q", "batch",
                                          "gMi", "gPn", "slots")] + [("slot_stride", C.c_int64)]


class Tn2UnitArgs(C.Structure):
    """tmdnet_tn2_unit_args (include/tmdnet_amd.h): one kernel of the TensorNet2 path on caller-built operands, tmdnet_debug_tn2."""
    _fields_ = [(n, C.c_int32) for n in ("op", "N", "B", "F", "P", "E", "qd", "QC", "box_mode")] + \
               [(n, C.c_float) for n in ("cut", "eps_solvent", "scale")] + [("slot_stride", C.c_int64)] + \
               [("slot_arrays_out", C.POINTER(C.c_int32))] + \
               [(n, C.c_void_p) for n in ("rowptr", "col", "epair", "counts", "mstart", "mend", "batch", "erev", "eid", "pair_edge",
                                          "X", "g_feat", "feat", "G", "out", "Qmol", "g_c", "charges", "FuQ", "g_out",
                                          "Ap", "Bt", "Cs", "C", "pre1", "he1", "Ce", "gMi", "Pn", "pre3", "g_pre3", "slots",
                                          "g_pre1", "gB", "gCs", "gAp", "dAp", "dC", "gd", "pos", "box", "wq", "ec", "g_q", "fpos")]


class EtUnitArgs(C.Structure):
    """tmdnet_et_unit_args (include/tmdnet_amd.h): one edge-sweep kernel of the Equivariant Transformer on caller-built operands,
    tmdnet_debug_et."""
    _fields_ = [(n, C.c_int32) for n in ("op", "kernel", "N", "B", "P", "E", "F", "hd", "Wd", "dk_off", "dv_off", "vector_cutoff",
                                         "pair_bf16", "skip_prep", "slot_min", "mailbox", "sync_every", "nw")] + \
               [("min_fill", C.c_float), ("slot_stride", C.c_int64), ("dir_stride", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("rowptr", "col", "epair", "esign", "counts", "pair_i", "pair_j", "prhat", "batch",
                                          "C", "dC", "qkv", "vec", "dkv", "tkv", "g_xagg", "g_vagg", "meta", "tile_start", "erec",
                                          "xagg", "vagg", "g_qkv", "g_vec", "gd2", "gr2", "gd_extra", "gd", "g_rhat",
                                          "z", "emb", "embN", "Wn", "dWn", "g_xcat", "xcat", "gEN",
                                          "slots", "self_rows", "self_sum", "pre", "g_pre")]


class PairPriors(C.Structure):
    """tmdnet_pair_priors (include/tmdnet_amd.h): flags, unit scales and host tables of the ZBL / D2 pair priors."""
    _fields_ = [("flags", C.c_int32), ("max_z", C.c_int32)] + \
               [(n, C.c_double) for n in ("zbl_cutoff", "zbl_distance_scale", "zbl_energy_scale", "d2_cutoff", "d2_distance_scale",
                                          "d2_energy_scale")] + \
               [(n, C.c_void_p) for n in ("zbl_z", "zbl_z23", "d2_sqrt_c6", "d2_rr")]


class CommitteeGate(C.Structure):
    """tmdnet_committee_gate (include/tmdnet_amd.h): thresholds, the loop's MD workspace and the buffers of the flagged molecules."""
    _fields_ = [("flags", C.c_int32), ("flag_above", C.c_float), ("stop_above", C.c_float)] + \
               [(n, C.c_void_p) for n in ("md_ws", "flagged_at", "flagged_dev", "flagged_atom", "flagged_pos")]


class HopArgs(C.Structure):
    """tmdnet_hop_args (include/tmdnet_amd.h): the parameters and the device buffers of a minima-hopping step."""
    _fields_ = [(n, C.c_double) for n in ("dt_max", "f_inc", "f_dec", "alpha0", "f_alpha", "max_step", "fmax", "dt0", "beta1", "beta2",
                                          "beta3", "alpha1", "alpha2", "rmsd_tol", "energy_tol")] + \
               [("seed", C.c_uint64), ("dt", C.c_float)] + \
               [(n, C.c_int32) for n in ("n_min", "mdmin", "md_steps", "opt_steps", "capacity", "align")] + \
               [(n, C.c_void_p) for n in ("pos", "vel", "forces", "energy", "hk", "mass", "sig", "fixed", "batch", "forces_keep",
                                          "cur_pos", "best_pos", "ring_pos", "ring_energy", "ring_found", "ring_visits", "kT", "ediff",
                                          "cur_energy", "best_energy", "phase", "counters", "epot_row", "fmax_row", "ekin_row",
                                          "phase_row", "outcome_row", "sums_row", "coef_row")]


class ObserveSpec(C.Structure):
    """tmdnet_md_observe_spec (include/tmdnet_amd.h): what the MD loop's observer records and how large its arrays are."""
    _fields_ = [("every", C.c_int32), ("frame_capacity", C.c_int32), ("frame_velocities", C.c_int32), ("n_pair_types", C.c_int32),
                ("bins", C.c_int32), ("r_max2", C.c_float), ("inv_dr", C.c_float), ("n_msd_groups", C.c_int32),
                ("n_vacf_groups", C.c_int32), ("lags", C.c_int32), ("msd_capacity", C.c_int64)]


# limits of the observer (tn_obs::kMax* of csrc/tn_observe_math.h) and the tile of its pair sweep
OBSERVE_MAX_TYPES, OBSERVE_MAX_BINS, OBSERVE_MAX_LAGS, OBSERVE_TILE = 4, 1024, 256, 256

# flags of tmdnet_set_pair_priors and the brute-force limit of the pass (TMDNET_PRIOR_* in the header)
PRIOR_ZBL, PRIOR_D2, PRIOR_MAX_MOLECULE_ATOMS = 1, 2, 32768
# limit and gate flags of the committee pass (TMDNET_COMMITTEE_* in the header)
COMMITTEE_MAX_MEMBERS, COMMITTEE_FLAG, COMMITTEE_STOP = 16, 1, 2
# ops of tmdnet_debug_tn2 (TMDNET_TN2_* in the header)
(TN2_EDGE_REVERSE, TN2_CP_FEAT, TN2_CP_FEAT_BWD, TN2_QEQ_FWD, TN2_QEQ_BWD, TN2_EDGE_PRE1, TN2_EDGE_GW, TN2_EDGE_REDUCE, TN2_PAIR_GD,
 TN2_COULOMB) = range(10)
# ops and kernel selectors of tmdnet_debug_et (TMDNET_ET_* in the header)
(ET_OP_QUERY, ET_OP_TILE_PREP, ET_OP_ATTN_FWD, ET_OP_ATTN_BWD, ET_OP_PAIR_COMBINE, ET_OP_NBR_EMBED, ET_OP_NBR_EMBED_BWD,
 ET_OP_TRAIN_NBR, ET_OP_TRAIN_FILTER, ET_OP_TRAIN_GPRE) = range(10)
ET_AUTO, ET_ROW_GENERIC, ET_ROW_PIPELINED, ET_TILE = range(4)
# sweeps and kernels of tmdnet_debug_message (TMDNET_MSG_* in the header)
MSG_OP_FWD, MSG_OP_ADJ, MSG_OP_GD, MSG_OP_DUAL = range(4)
(MSG_AUTO, MSG_FWD_ROW, MSG_FWD_SPLIT, MSG_FWD_TILE, MSG_ADJ_ROW, MSG_ADJ_SPLIT, MSG_GD_ROW, MSG_GD_SPLIT, MSG_GD_TILE, MSG_DUAL,
 MSG_DUAL_ACC) = range(11)
MSG_DUAL_SPLIT3 = 16
# flags and routes of tmdnet_debug_gemm_ex (TMDNET_GEMM_* in the header)
GEMM_ACT_SILU, GEMM_MUL_AUX, GEMM_MUL_DSILU_AUX, GEMM_ACCUM, GEMM_ROWSCALE = 1, 2, 4, 8, 16
(GEMM_ROUTE_NONE, GEMM_ROUTE_SKINNY4, GEMM_ROUTE_SKINNY8, GEMM_ROUTE_TILES_128X128, GEMM_ROUTE_TILES_128X64,
 GEMM_ROUTE_TILES_128X32, GEMM_ROUTE_SB1_128, GEMM_ROUTE_SB1_64) = range(8)
# prologues and epilogues of tmdnet_debug_tlin9
TL9_PRO_PLAIN, TL9_PRO_NORM, TL9_PRO_UPDBWD = 0, 1, 2
TL9_EPI_PLAIN, TL9_EPI_MULGATE, TL9_EPI_UPDATE, TL9_EPI_NORMBWD, TL9_EPI_NORMBWD_GATE, TL9_EPI_EMBBWD = range(6)
# modes of tmdnet_vib_seed / tmdnet_vib_gather / tmdnet_vib_finish (TMDNET_VIB_* in the header)
VIB_SEED, VIB_PLUS, VIB_MINUS = range(3)
VIB_ANALYTIC, VIB_CENTRAL = range(2)
VIB_PROJECT_NONE, VIB_PROJECT_TRANS, VIB_PROJECT_TRANS_ROT = range(3)
VIB_INFO = 8

_lib = None


def lib():
    """Load the shared library (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first (python __graft_entry__.py). "
            "torchmdnet_amd has no CPU or eager-PyTorch fallback."
        )
    L = C.CDLL(LIB_PATH)
    # the ABI revision first: binding the argtypes of a symbol that a stale library lacks would end in a bare AttributeError
    abi = int(re.search(r"#define\s+TMDNET_ABI_VERSION\s+(\d+)", open(HEADER_PATH).read()).group(1))
    if L.tmdnet_abi_version() != abi:
        raise ImportError(f"{LIB_PATH} has ABI revision {L.tmdnet_abi_version()}, include/tmdnet_amd.h declares {abi}: rebuild")
    vp, i64, i32, f32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_size_t
    L.tmdnet_create.argtypes = [C.POINTER(HParams), C.POINTER(vp)]
    L.tmdnet_create_et.argtypes = [C.POINTER(EtHParams), C.POINTER(vp)]
    L.tmdnet_create_tn2.argtypes = [C.POINTER(Tn2HParams), C.POINTER(vp)]
    L.tmdnet_destroy.argtypes = [vp]
    L.tmdnet_last_error.argtypes = [vp]
    L.tmdnet_last_error.restype = C.c_char_p
    L.tmdnet_version.restype = C.c_char_p
    L.tmdnet_set_param.argtypes = [vp, C.c_char_p, vp, i64]
    L.tmdnet_finalize_params.argtypes = [vp]
    L.tmdnet_update_params_device.argtypes = [vp, vp, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(vp)]
    L.tmdnet_num_params.argtypes = [vp]
    L.tmdnet_param_name.argtypes = [vp, C.c_int, C.POINTER(i64)]
    L.tmdnet_param_name.restype = C.c_char_p
    L.tmdnet_set_option.argtypes = [vp, C.c_char_p, C.c_double]
    L.tmdnet_get_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double)]
    L.tmdnet_graph_workspace_bytes.argtypes = [vp, i64, i64, C.POINTER(sz)]
    L.tmdnet_build_graph.argtypes = [vp, vp, vp, sz, i64, i64, vp, vp, vp, vp, i32, C.POINTER(i64)]
    L.tmdnet_set_cell_grid.argtypes = [vp, i32, i32, i32]
    L.tmdnet_set_atom_weights.argtypes = [vp, vp]
    L.tmdnet_set_halo_exchange.argtypes = [vp, HALO_EXCHANGE_FN, vp]
    L.tmdnet_build_graph_static.argtypes = [vp, vp, vp, sz, i64, i64, vp, vp, vp, vp, i32]
    L.tmdnet_graph_counts.argtypes = [vp, vp, vp, i64, i64, C.POINTER(i64)]
    L.tmdnet_graph_cell_grid.argtypes = [vp, vp, vp, i64, i64, C.POINTER(i64)]
    L.tmdnet_forward_workspace_bytes.argtypes = [vp, i64, i64, i64, i64, i32, C.POINTER(sz)]
    L.tmdnet_energy_forces.argtypes = [vp, vp, vp, vp, sz, i64, i64, i64, vp, vp, vp, i32, vp, vp]
    L.tmdnet_virial_workspace_bytes.argtypes = [vp, i64, i64, C.POINTER(sz)]
    L.tmdnet_energy_forces_virial.argtypes = [vp, vp, vp, vp, sz, vp, sz, i64, i64, i64, vp, vp, vp, i32, vp, vp, vp]
    L.tmdnet_neighbor_workspace_bytes.argtypes = [i64, i64, i64, C.POINTER(sz)]
    L.tmdnet_neighbor_pairs.argtypes = [vp, vp, sz, i64, i64, vp, vp, vp, i32, f32, f32, i64, i32, i32, i32, vp, vp, vp, vp]
    L.tmdnet_neighbor_grad.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, vp]
    f64 = C.c_double
    L.tmdnet_neighbor_pairs_f64.argtypes = [vp, vp, sz, i64, i64, vp, vp, vp, i32, f64, f64, i64, i32, i32, vp, vp, vp, vp]
    L.tmdnet_neighbor_grad_f64.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, vp]
    L.tmdnet_profile_begin.argtypes = [vp, C.c_uint32]
    L.tmdnet_profile_end.argtypes = [vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i64)]
    L.tmdnet_profile_end_records.argtypes = [vp, vp, i64, C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                              C.POINTER(C.c_double), C.c_char_p, C.POINTER(i64)]
    L.tmdnet_profile_category_name.argtypes = [C.c_int]
    L.tmdnet_profile_category_name.restype = C.c_char_p
    L.tmdnet_debug_tensor.argtypes = [vp, vp, C.c_char_p, vp, i64]
    L.tmdnet_debug_graph.argtypes = [vp, vp, vp, i64, i64, C.c_char_p, vp, i64]
    L.tmdnet_debug_gemm_dual.argtypes =[vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, vp, vp, vp]
    L.tmdnet_debug_split_weight.argtypes = [vp, i64, i64, vp]
    L.tmdnet_debug_split_weight.restype = i64
    L.tmdnet_debug_gemm.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i32, vp]
    L.tmdnet_debug_gemm_ex.argtypes = [vp, C.POINTER(GemmExArgs), C.POINTER(i32)]
    L.tmdnet_debug_tlin9.argtypes = [vp, i32, i32, i64, i64] + [vp] * 11 + [i32, vp, vp, vp, vp, C.POINTER(i64)]
    L.tmdnet_debug_message.argtypes = [vp, C.POINTER(MessageArgs), C.POINTER(i32), C.POINTER(i32)]
    L.tmdnet_debug_message_fold.argtypes = [vp, C.POINTER(MessageFoldArgs)]
    L.tmdnet_debug_tn2.argtypes = [vp, C.POINTER(Tn2UnitArgs)]
    L.tmdnet_debug_et.argtypes = [vp, C.POINTER(EtUnitArgs), C.POINTER(i32)]
    L.tmdnet_param_grad_count.argtypes = [vp]
    L.tmdnet_param_grad_entry.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(i64)]
    L.tmdnet_param_grad_entry.restype = C.c_char_p
    L.tmdnet_train_workspace_bytes.argtypes = [vp, i64, i64, i64, C.POINTER(sz), C.POINTER(sz), C.POINTER(i64)]
    L.tmdnet_energy_param_grads.argtypes = [vp, vp, vp, vp, sz, vp, sz, i64, i64, i64, vp, vp, vp, vp, vp, vp]
    L.tmdnet_force_param_workspace_bytes.argtypes = [vp, i64, i64, i64, C.POINTER(sz)]
    L.tmdnet_force_param_grads.argtypes = [vp, vp, vp, vp, sz, i64, i64, i64, vp, vp, vp, vp, vp, vp]
    L.tmdnet_loss_param_grads.argtypes = [vp, vp, vp, vp, sz, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp]
    L.tmdnet_hvp_debug_tensor.argtypes = [vp, vp, C.c_char_p, vp, i64]
    L.tmdnet_set_output_head.argtypes = [vp, i32]
    u64 = C.c_uint64
    L.tmdnet_md_workspace_bytes.argtypes = [i64, i64, C.POINTER(sz)]
    L.tmdnet_md_reset.argtypes = [vp, vp, u64]
    L.tmdnet_md_advance.argtypes = [vp, vp, vp, vp, i64, i64, i32, vp, vp, vp, vp, vp, vp, vp, f32, f32, f32, u64, vp, vp, vp, vp]
    L.tmdnet_md_status.argtypes = [vp, vp, C.POINTER(u64)]
    L.tmdnet_md_barostat_workspace_bytes.argtypes = [i64, C.POINTER(sz)]
    L.tmdnet_md_barostat.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, vp, vp, vp, vp, f32, vp, vp, i32, vp, vp, f64, f64, f64, f64, f64,
                                     u64, vp, vp, vp]
    L.tmdnet_md_barostat_cell_workspace_bytes.argtypes = [i64, i64, C.POINTER(sz)]
    L.tmdnet_md_barostat_cell.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, vp, vp, vp, vp, vp, f32, vp, vp, i32, vp, f64, f64, f64, f64,
                                          f64, u64, i32, i32, vp, vp, vp, vp]
    L.tmdnet_md_thermostat_workspace_bytes.argtypes = [i64, i32, C.POINTER(sz)]
    L.tmdnet_md_thermostat.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp, f64, f64, i32, i32, f64, u64,
                                       vp, vp]
    L.tmdnet_md_exchange_workspace_bytes.argtypes = [i64, i32, C.POINTER(sz)]
    L.tmdnet_md_exchange.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, i64, vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp]
    L.tmdnet_md_bias_workspace_bytes.argtypes = [i64, i32, i32, i32, i64, C.POINTER(sz)]
    L.tmdnet_md_bias_reset.argtypes = [vp, vp, u64, u64]
    L.tmdnet_md_bias.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32,
                                 f64, f64, f64, f64, f64, i64, i32, i64, vp, vp, vp, vp]
    L.tmdnet_md_observe_workspace_bytes.argtypes = [i64, i64, C.POINTER(ObserveSpec), C.POINTER(sz)]
    L.tmdnet_md_observe_start.argtypes = [vp, vp, i64, i64, C.POINTER(ObserveSpec), u64, vp]
    L.tmdnet_md_observe.argtypes = [vp, vp, vp, vp, vp, i64, i64, C.POINTER(ObserveSpec), vp, vp, vp, vp, i32, vp, vp, vp, i64]
    L.tmdnet_md_constraints_workspace_bytes.argtypes = [i64, i64, i64, C.POINTER(sz)]
    L.tmdnet_md_advance_constrained.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, vp, vp, vp, vp, vp, vp, vp, f32, f32, f32, u64, vp, vp,
                                                vp, vp, i64, i64, vp, vp, vp, vp, f64, i32]
    L.tmdnet_min_workspace_bytes.argtypes = [i64, i64, C.POINTER(sz)]
    L.tmdnet_min_reset.argtypes = [vp, vp, u64, f64, f64]
    L.tmdnet_min_advance.argtypes = [vp, vp, vp, vp, i64, i64, i32, vp, vp, vp, vp, vp, vp, vp, f64, i32, f64, f64, f64, f64, f64, f64,
                                     vp, vp, vp, vp, vp, vp, vp]
    L.tmdnet_min_status.argtypes = [vp, vp, C.POINTER(u64)]
    L.tmdnet_min_workspace_bytes_cell.argtypes = [i64, i64, C.POINTER(sz)]
    L.tmdnet_min_reset_cell.argtypes = [vp, vp, i64, i64, u64, f64, f64, vp, vp, vp, vp, vp]
    L.tmdnet_min_advance_cell.argtypes = L.tmdnet_min_advance.argtypes + [vp, vp, vp, vp, vp, vp, C.POINTER(f64), i32, f64, vp, vp, vp]
    L.tmdnet_min_status_cell.argtypes = [vp, vp, C.POINTER(u64)]
    L.tmdnet_lbfgs_workspace_bytes.argtypes = [i64, i64, i32, C.POINTER(sz)]
    L.tmdnet_lbfgs_layout.argtypes = [i64, i64, i32, C.POINTER(i64)]
    L.tmdnet_lbfgs_reset.argtypes = [vp, vp, u64]
    L.tmdnet_lbfgs_advance.argtypes = [vp, vp, vp, vp, i64, i64, i32, vp, vp, vp, vp, vp, vp, vp, i32, f64, f64, f64, f64,
                                       vp, vp, vp, vp, vp, vp, vp]
    L.tmdnet_lbfgs_status.argtypes = [vp, vp, C.POINTER(u64)]
    L.tmdnet_neb_workspace_bytes.argtypes = [i64, i64, i64, C.POINTER(sz)]
    L.tmdnet_neb_reset.argtypes = [vp, vp, u64, f64, f64, i32]
    L.tmdnet_neb_advance.argtypes = [vp, vp, vp, vp, i64, i64, i64, i32, vp, vp, vp, vp, vp, vp, f64, i32, f64, f64, f64, f64, f64, f64,
                                     f64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tmdnet_neb_status.argtypes = [vp, vp, C.POINTER(u64)]
    L.tmdnet_dimer_workspace_bytes.argtypes = [i64, i64, C.POINTER(sz)]
    L.tmdnet_dimer_reset.argtypes = [vp, vp, u64, f64, f64, i32]
    L.tmdnet_dimer_advance.argtypes = [vp, vp, vp, vp, i64, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, f64, i32, f64, f64, f64, f64, f64,
                                       f64, f64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tmdnet_dimer_status.argtypes = [vp, vp, C.POINTER(u64)]
    L.tmdnet_irc_workspace_bytes.argtypes = [i64, i64, i64, C.POINTER(sz)]
    L.tmdnet_irc_reset.argtypes = [vp, vp, u64, f64]
    L.tmdnet_irc_advance.argtypes = [vp, vp, vp, vp, i64, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, f64, f64, f64, f64, f64,
                                     vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tmdnet_irc_status.argtypes = [vp, vp, C.POINTER(u64)]
    L.tmdnet_scan_workspace_bytes.argtypes = [i64, i64, C.POINTER(sz)]
    L.tmdnet_scan_reset.argtypes = [vp, vp, i64, i64, u64, f64, f64]
    L.tmdnet_scan_advance.argtypes = [vp, vp, vp, vp, i64, i64, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, f64, i32, f64, i32, f64,
                                      f64, f64, f64, f64, f64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tmdnet_scan_status.argtypes = [vp, vp, C.POINTER(u64)]
    L.tmdnet_hop_workspace_bytes.argtypes = [i64, i64, i32, C.POINTER(sz)]
    L.tmdnet_hop_reset.argtypes = [vp, vp, i64, i64, C.POINTER(HopArgs), u64, vp, vp, i32]
    L.tmdnet_hop_advance.argtypes = [vp, vp, vp, vp, i64, i64, C.POINTER(HopArgs)]
    L.tmdnet_hop_status.argtypes = [vp, vp, C.POINTER(u64)]
    L.tmdnet_vib_workspace_bytes.argtypes = [i64, i64, C.POINTER(sz)]
    L.tmdnet_vib_seed.argtypes = [vp, i32, i64, i64, i64, i64, vp, vp, vp, vp, f32, vp]
    L.tmdnet_vib_gather.argtypes = [vp, i32, i64, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tmdnet_vib_finish.argtypes = [vp, vp, sz, i64, i64, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tmdnet_set_pair_priors.argtypes = [vp, C.POINTER(PairPriors)]
    L.tmdnet_pair_priors_workspace_bytes.argtypes = [vp, i64, i64, C.POINTER(sz)]
    L.tmdnet_pair_priors_add.argtypes = [vp, vp, vp, sz, i64, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.tmdnet_debug_prior.argtypes = [vp, vp, vp, sz, i64, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.tmdnet_committee_workspace_bytes.argtypes = [i64, i64, C.POINTER(sz)]
    L.tmdnet_committee_reset.argtypes = [vp, vp, i64]
    L.tmdnet_committee_reduce.argtypes = [vp, vp, sz, i32, C.POINTER(vp), C.POINTER(vp), i64, i64, vp, vp, vp, vp, vp, vp, vp, vp,
                                          C.POINTER(vp), C.POINTER(vp), C.POINTER(CommitteeGate)]
    L.tmdnet_committee_latch.argtypes = [vp, vp, i64, i64, vp, vp, vp, C.POINTER(CommitteeGate)]
    L.tmdnet_committee_status.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    for name in declared_symbols():
        fn = getattr(L, name)
        if fn.restype is C.c_int:
            fn.restype = C.c_int
    _lib = L
    return L


# tmdnet_halo_exchange_fn (include/tmdnet_amd.h): (user, stage, rows, n_rows, row_floats, perm, stream) -> 0 on success
HALO_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p)


def declared_symbols():
    """Every function declared in include/tmdnet_amd.h."""
    with open(HEADER_PATH) as fh:
        txt = fh.read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(tmdnet_[a-z0-9_]+)\s*\(", txt)))


def check_symbols():
    L = lib()
    missing = [s for s in declared_symbols() if not hasattr(L, s)]
    if missing:
        raise ImportError(f"libtmdnet_amd.so does not export: {missing}")
    return declared_symbols()
