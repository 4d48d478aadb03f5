/* tmdnet_amd.h -- C ABI of the MI355X-native TensorNet energy+force engine (libtmdnet_amd.so).
 *
 * Drop-in boundary.  The reference has no C FFI of its own on this path:
 * its "native" seam is a set of torch custom ops written in NVIDIA Warp
 * (torchmdnet/extensions/ops.py:14-106, the files under torchmdnet/extensions/warp_ops/) below the Python
 * surface create_model / load_model / TorchMD_Net.forward (torchmdnet/models/model.py:21,208,530).
 * This header is what a binding for that path binds instead: plain pointers and sizes, no torch
 * types.  The host side in torchmd-net_amd/torchmdnet_amd/ calls it through ctypes (see
 * INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - every `const float*` / `const int64_t*` data pointer is a DEVICE pointer (HIP, gfx950) unless
 *     the parameter name ends in `_host`; all tensors are dense row-major fp32 / int64.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).  Calls enqueue work and return;
 *     only tmdnet_build_graph synchronises the stream (it reads back three integers, the analogue
 *     of the reference's `resize_to_fit` host sync, torchmdnet/models/utils.py:303-307).
 *   - no hidden device allocation happens inside build_graph / energy_forces: the caller owns both
 *     workspaces (size them with the *_workspace_bytes queries).
 *   - a handle is re-entrant across handles but not thread-safe on one handle.
 *   - return value: 0 on success, a TMDNET_ERR_* code otherwise; tmdnet_last_error() gives text.
 */
#ifndef TMDNET_AMD_H
#define TMDNET_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMDNET_OK 0
#define TMDNET_ERR_INVALID 1   /* bad argument / unknown parameter / wrong size; also: atomic number or molecule
                                  index out of range (the reference's nn.Embedding / scatter raise there) */
#define TMDNET_ERR_HIP 2       /* a HIP runtime call failed */
#define TMDNET_ERR_OVERFLOW 3  /* more neighbour pairs than max_num_neighbors * n_atoms:
                                  the reference raises RuntimeError here (models/utils.py:297-300) */
#define TMDNET_ERR_WORKSPACE 4 /* caller workspace too small */
#define TMDNET_ERR_STATE 5     /* call order violated (e.g. parameters not finalised) */

typedef struct tmdnet_model tmdnet_model; /* opaque */

/* Hyper-parameters of TensorNet + Scalar head: the subset of the reference's create_model argument
 * dict that the path depends on (torchmdnet/models/model.py:35-60,96-105,134-152). */
typedef struct tmdnet_hparams {
  int32_t hidden_channels;   /* embedding_dimension (F) */
  int32_t num_layers;        /* interaction layers (L) */
  int32_t num_rbf;           /* ExpNormal radial basis size (K) */
  int32_t max_z;             /* rows of the atom-type embedding */
  int32_t max_num_neighbors; /* pair capacity = max_num_neighbors * n_atoms (tensornet.py:281-290) */
  int32_t group_o3;          /* 1: O(3) (Y M + M Y), 0: SO(3) (2 Y M)   (tensornet.py:788-793) */
  int32_t head_hidden;       /* Scalar head hidden width (F/2, output_modules.py:96-103) */
  int32_t has_atomref;       /* 1: an "atomref" table [max_z] is added per atom (priors/atomref.py:93-96) */
  float cutoff_lower;
  float cutoff_upper;
} tmdnet_hparams;

/* Hyper-parameters of the Equivariant Transformer + EquivariantScalar head (reference
 * torchmdnet/models/torchmd_et.py:84-103, model.py:62-81,134-135).  Activations are SiLU (activation, attn_activation). */
typedef struct tmdnet_et_hparams {
  int32_t hidden_channels;    /* embedding_dimension (F) */
  int32_t num_layers;         /* attention layers */
  int32_t num_rbf;            /* ExpNormal radial basis size (K) */
  int32_t max_z;
  int32_t max_num_neighbors;  /* pair capacity = max_num_neighbors * n_atoms */
  int32_t num_heads;          /* F / num_heads must be a power of two <= 64 */
  int32_t neighbor_embedding; /* 1: NeighborEmbedding (models/utils.py:45-117) */
  int32_t vector_cutoff;      /* 1: cutoff on the values, 0: on the attention weights (torchmd_et.py:395-401) */
  int32_t distance_influence; /* bit 0: keys (dk_proj), bit 1: values (dv_proj) */
  int32_t has_atomref;
  float cutoff_lower;
  float cutoff_upper;
} tmdnet_et_hparams;

/* Hyper-parameters of TensorNet2 + ScalarPlusWeightedCoulomb (AceFF-2.0; reference
 * torchmdnet/models/tensornet2.py:160-330, output_modules.py:344-441, model.py:106-152).  TensorNet with per-atom charge
 * channels: a ChargePredict head after the embedding and after every layer (invariants -> LayerNorm -> MLP -> charge
 * equilibration to the molecule's total charge `q`), the next layer's edge MLP takes [phi(d), c_i, c_j], and the head adds
 * the damped pair Coulomb energy of all (num_layers + 1) * q_dim charge channels, weighted by `output_model.qweights`. */
typedef struct tmdnet_tn2_hparams {
  int32_t hidden_channels, num_layers, num_rbf, max_z, max_num_neighbors, group_o3, head_hidden, has_atomref;
  int32_t q_dim;                 /* charge channels per ChargePredict head, (num_layers + 1) * q_dim <= 64 */
  float cutoff_lower, cutoff_upper;
  float coulomb_cutoff;          /* <= 0: all pairs of a molecule (no PBC); > 0: reaction field inside this cutoff */
  float coulomb_epsilon_solvent; /* reaction-field dielectric constant (reference default 78.3) */
} tmdnet_tn2_hparams;

/* ---- lifecycle ------------------------------------------------------------------------------- */
int tmdnet_create(const tmdnet_hparams* hp, tmdnet_model** out);
/* TensorNet2 handle: parameters by the reference's state-dict keys, every other entry point shared.  tmdnet_build_graph must
 * be given the positions / box it should use for the Coulomb sum as well (it keeps the pointers until tmdnet_energy_forces). */
int tmdnet_create_tn2(const tmdnet_tn2_hparams* hp, tmdnet_model** out);
/* Equivariant Transformer handle: every other entry point (parameters by state-dict key, graph, energy_forces with
 * q = NULL, workspaces, profiling) is shared with the TensorNet handle. */
int tmdnet_create_et(const tmdnet_et_hparams* hp, tmdnet_model** out);
int tmdnet_destroy(tmdnet_model* m);
const char* tmdnet_last_error(const tmdnet_model* m);
const char* tmdnet_version(void);
/* ABI revision of this header: bumped whenever an exported signature or struct layout changes (3: `z` in
 * tmdnet_build_graph[_static], `strategy` in tmdnet_neighbor_pairs).  A binding compares its compile-time
 * TMDNET_ABI_VERSION with the loaded library's tmdnet_abi_version() before its first call. */
#define TMDNET_ABI_VERSION 10
int tmdnet_abi_version(void);

/* Output head of the handle (ABI 10): TMDNET_HEAD_SCALAR (the default; energies), TMDNET_HEAD_DIPOLE_MOMENT (|| sum (q_i (r_i - c) +
 * std v_i) + mean ||, reference output_modules.py:166-245), TMDNET_HEAD_SPATIAL_EXTENT (sum q_i ||r_i - c||^2 + mean,
 * output_modules.py:248-297), TMDNET_HEAD_VECTOR (sum std v_i + mean, Equivariant Transformer only, output_modules.py:300-323).
 * q_i is the head's scalar output times std, v_i the vector output of the Equivariant Transformer's second gated block (0 on
 * TensorNet), c the molecule's centre of mass with the masses of the parameter "output_model.atomic_mass" ([TMDNET_MASS_TABLE_SIZE],
 * indexed by z), r_i the positions given to tmdnet_build_graph* (not wrapped into the box; the pointer must still be valid at
 * tmdnet_energy_forces, as for TensorNet2).  Call after tmdnet_create* and before the first tmdnet_num_params / tmdnet_set_param: the
 * parameter list changes (the dipole and spatial-extent heads add "output_model.atomic_mass"; on the Equivariant Transformer the
 * spatial-extent head is the MLP "output_model.output_network.layers.{0,2}.*" instead of the gated blocks).  The energy output of
 * tmdnet_energy_forces then holds the property: n_mol floats, 3 n_mol for TMDNET_HEAD_VECTOR; the forces are minus the position
 * gradient of the sum of its components.  TMDNET_ERR_INVALID for TensorNet2, the vector head on TensorNet, or an unknown kind.  The
 * property heads take neither atom weights nor the halo exchange, and have no parameter-gradient or second-order pass
 * (TMDNET_ERR_INVALID from those entries). */
#define TMDNET_HEAD_SCALAR 0
#define TMDNET_HEAD_DIPOLE_MOMENT 1
#define TMDNET_HEAD_SPATIAL_EXTENT 2
#define TMDNET_HEAD_VECTOR 3
#define TMDNET_MASS_TABLE_SIZE 119
int tmdnet_set_output_head(tmdnet_model* m, int32_t kind);

/* Parameters are addressed by the reference's state-dict keys without the "model." prefix
 * (SURVEY.md Appendix A), e.g. "representation_model.layers.0.linears_scalar.2.weight", plus
 * "mean", "std" and "atomref".  `data_host` is HOST memory, row-major, `numel` floats; it is copied.
 * tmdnet_finalize_params checks that every tensor is present with the expected size, builds the
 * transposed copies used by the reverse pass and uploads one packed device buffer.  It marks the radial
 * tables stale: the first tmdnet_energy_forces after it rebuilds them (blocking, NULL stream, tens of ms)
 * and returns TMDNET_ERR_STATE if its stream is being captured at that moment. */
int tmdnet_set_param(tmdnet_model* m, const char* name, const float* data_host, int64_t numel);
int tmdnet_finalize_params(tmdnet_model* m);
/* Device-side parameter update (training loops; TensorNet and TensorNet2): `dev_ptrs[c]` is the fp32, contiguous DEVICE copy of
 * state-dict tensor `names[c]` (any subset; "mean" / "std" excluded - they are host-read kernel arguments).  Needs one
 * tmdnet_set_param + tmdnet_finalize_params round first (shapes, layout, host-built images).  Enqueues on `stream`: one gather
 * kernel rewrites the packed parameter buffer from the caller's tensors (the mapping is learnt once by running the packing on
 * index tags), then the split-bf16 images and the per-species tables are rebuilt by kernels; nothing crosses PCIe except a
 * pointer table, no synchronisation.  The caller's tensors must stay valid until the stream reaches this point.  Afterwards
 * the radial tables are stale (rebuilt by the first call that uses them) and the radial-basis embedding stays off until the
 * next full tmdnet_finalize_params (its weight images are made on the host).  Evaluations that used the handle on OTHER
 * streams must have finished (same rule as tmdnet_finalize_params, which additionally blocks the host). */
int tmdnet_update_params_device(tmdnet_model* m, void* stream, int32_t count, const char* const* names, const float* const* dev_ptrs);
/* number of parameter tensors the model expects; name of the idx-th one and its element count */
int tmdnet_num_params(const tmdnet_model* m);
const char* tmdnet_param_name(const tmdnet_model* m, int idx, int64_t* numel);

/* ---- radial tables of the per-pair functions --------------------------------------------------------------------
 * Q_c(d) = P_c phi(d) + b_c and every layer's edge MLP w^l(d) (reference tensornet.py:558-560, 738-743) depend on the pair
 * distance only.  tmdnet_finalize_params evaluates them and their d/dd once on a uniform grid in double precision,
 * stores fp32 rows, and verifies the step's cubic Hermite interpolation against the fp64 evaluation at every interval
 * midpoint (bounds: 5e-7 of the table's largest value, 2e-6 of its largest slope; the grid is refined 8192 -> 65536
 * intervals until they hold, else the tables stay off) and tmdnet_energy_forces then interpolates per pair instead of running the pair-row
 * GEMMs, when the system has at least `edge_table_min_pairs` pairs (default 1024: single systems from about 100 atoms on).  TMDNET_EDGE_TABLE=0 in the
 * environment disables the tables (direct GEMMs every step).
 * Options: "edge_table_min_pairs"; "pair_rows_bf16" (Equivariant Transformer handle only; 1: the per-pair distance-filter
 * rows silu(dk_proj phi) | silu(dv_proj phi) and their d/dd - reference torchmd_et.py:375-415 - are written by the table
 * interpolation as bf16 and widened when the attention sweeps load them; products and sums stay fp32; 2: a developer and test mode - the rows are rounded by the same conversion and widened back into
 * fp32 rows, so the fp32-row sweeps run on the values the bf16-row sweeps read, and the sweep generation is chosen with the bf16
 * rows' tile-fill threshold; default 0; tmdnet_get_info returns the value set).  tmdnet_debug_tensor "dkv<l>" / "tkv<l>" copy layer l's
 * value / tangent rows of the last call: (pairs + 1) * Wd floats, or half as many floats holding the raw bf16 pairs with option 1.  Info: "edge_table_T" (0 = off), "edge_table_err_value", "edge_table_err_slope"
 * (measured at the midpoints), "edge_table_min_pairs".
 * "recompute_pair_rows" (TensorNet handle; default 0): 1 = the message sweeps interpolate a layer's per-pair row from its table
 * themselves (12 table loads per edge instead of 3, or 6 in the reverse sweep) and the rows w^l, d w^l / dd, the distance
 * projections' rows and the direct evaluation's activations get NO workspace: tmdnet_forward_workspace_bytes drops from
 * ~12.6 KB to ~0.1 KB per pair, which is what lets a 10^6-atom periodic box fit one 288 GB device.  Same arithmetic as the stored
 * rows (one definition, csrc/tn_interp.h): energies and forces are bit-identical.  Needs the tables (verified, not switched
 * off); tmdnet_energy_forces reports TMDNET_ERR_STATE otherwise.  tmdnet_forward_workspace_bytes plans for the embedding form
 * of the graph this handle built LAST (query it after tmdnet_build_graph of the same system, as the Python host does); a plan made
 * for another graph is refused with TMDNET_ERR_WORKSPACE, never overrun.
 * "fold_node_adjoint" (TensorNet handle; default 1): when the graph came from tmdnet_build_graph on the brute-force path, `batch`
 * was sorted and no molecule lies across a multiple of 64 atoms (counts_host[7] == 0), and the step takes the tile sweeps
 * (TMDNET_MSG_GD_TILE) without halo exchange, parameter gradients or "recompute_pair_rows", the reverse tile sweep computes the
 * adjoint of the group product in its prologue instead of reading it from a kernel of its own.  Same arithmetic (one definition,
 * csrc/tn_common.h): forces are bit-identical with 0 and 1.  Info "message_adjoint_fold_last": 1 when the last call ran that way. */
int tmdnet_set_option(tmdnet_model* m, const char* name, double value);
int tmdnet_get_info(const tmdnet_model* m, const char* name, double* value);

/* ---- phase A: neighbour graph ------------------------------------------------------------------
 * Replaces OptimizedDistance.forward + get_neighbor_pairs_kernel + graph_transform
 * (torchmdnet/models/utils.py:233-313, extensions/ops.py:14, warp_ops/graph_transform.py:160-179).
 * Brute-force pair search restricted to each molecule, self loops included, both directions,
 * optional triclinic minimum image (box_mode 1: one [3,3] box, 2: one box per molecule [B,3,3]).
 * Produces a deterministic pair list + symmetric CSR inside `graph_ws`.
 * counts_host[0] = number of undirected pairs P, [1] = number of directed edges incl. self loops E,
 * [2] = overflow flag, [3] = 1 if `batch` was not sorted (slow path), [4] = 1 if an atomic number was outside
 * [0, max_z), [5] = 1 if a molecule index was outside [0, n_mol); [6] = species count (embedding in the radial basis),
 * [7] = 1 if an atom i > 0, i % 64 == 0, shares its molecule with atom i - 1 (a molecule across a 64-row tile boundary).
 * `z` (int64 [n_atoms], may be NULL) is validated here, in the same read-back: out-of-range values return
 * TMDNET_ERR_INVALID before any table is indexed with them (the reference's nn.Embedding raises IndexError,
 * tensornet.py:473); a validated copy in the graph's internal atom order is kept in `graph_ws` and used by
 * tmdnet_energy_forces.  With z = NULL nothing is checked and tmdnet_energy_forces uses its own `z` argument as is.
 * Returns TMDNET_ERR_OVERFLOW when E > max_num_neighbors * n_atoms. */
int tmdnet_graph_workspace_bytes(const tmdnet_model* m, int64_t n_atoms, int64_t n_mol, size_t* bytes);
/* O(N) cell list (reference "cell" strategy: extensions/neighbor_utils.py:89-150, warp_kernels/neighbors_cell.py:17-153;
 * the reference handles orthorhombic boxes only; here any box in the reduced lower-triangular form a=(ax,0,0),
 * b=(bx,by,0), c=(cx,cy,cz) is taken, one box for the whole system).
 *   (0,0,0)   : always brute force (default);
 *   negative  : cell list whenever n_mol == 1 and box_mode == 1, with the grid n_axis = floor(w_axis / cutoff_upper)
 *               (w_axis = perpendicular width of the box along that axis) computed ON THE DEVICE from the box of
 *               each call -- no host copy of the box, and a captured HIP graph stays valid when the box changes (NPT);
 *   positive  : the same with an explicit grid (n_x*n_y*n_z <= 8*n_atoms, else brute force).
 * Any grid gives the same pair set as brute force (axes with fewer than 3 cells visit each cell once); atoms are
 * renumbered in cell order internally and forces are returned in the caller's order. */
int tmdnet_set_cell_grid(tmdnet_model* m, int32_t ncx, int32_t ncy, int32_t ncz);

/* Per-atom weights of the energy sum (ABI 5): E_mol = sum_i w_i e_i + mean, and the forces are minus the gradient of THAT sum.
 * `weights_dev` is a device vector of n_atoms floats in the caller's atom order (read by every later tmdnet_energy_forces on this
 * handle until it is reset with NULL; it must stay valid for as long as a captured HIP graph replays the call).  This is what a
 * domain decomposition of one large system needs (parallel.SpatialEvaluator): a rank evaluates its owned atoms (w = 1) inside a
 * halo of ghost copies (w = 0), and the ranks' forces add up to the whole system's.  The reference has no such argument: its
 * multi-GPU story stops at data parallelism over molecules.  TensorNet only (ET / TensorNet2 and the
 * parameter-gradient pass refuse a handle with weights set). */
int tmdnet_set_atom_weights(tmdnet_model* m, const float* weights_dev);

/* Per-layer halo exchange (ABI 8) for a domain decomposition whose halo is ONE cutoff deep (parallel.HaloExchangeEvaluator; the
 * reference has no counterpart).  A rank's local system is its owned atoms (weight 1) plus the ghost
 * copies within one cutoff of its domain (weight 0).  Every per-atom kernel of the step is local to a row, and a neighbour sweep
 * only gathers rows of neighbours, so the result on the owned atoms is exact as long as the ghost rows of the tensor each sweep
 * gathers hold their owners' values.  With a callback set, tmdnet_energy_forces (TensorNet inference, exact pair count) calls
 *     fn(user, stage, rows, n_rows, row_floats, perm, stream)
 * on the host, between enqueueing the kernel that writes `rows` ([n_rows][row_floats] floats on the device, n_rows = n_atoms) and
 * the sweep that gathers it: stage l = P_l of layer l (forward, row_floats = 9 F), 100 + l = the adjoint of layer l's message
 * (reverse, 9 F), 200 = the adjoint of the embedding sum (reverse, 10 F); 2 L + 1 calls per step.  The callback overwrites the
 * ghost rows with their owners' rows, ordered on `stream`.  Row r of `rows` belongs to the caller's atom perm[r] (perm == NULL:
 * to atom r; a device vector, valid during the call).  A non-zero return aborts the step with TMDNET_ERR_STATE.  The forces come
 * back for every local atom; those of the owned atoms are complete (no reduction over ranks), those of the ghosts are not.
 * fn == NULL switches the exchange off.  Not capturable: the callback runs at enqueue time.
 * Set together with the atom weights BEFORE tmdnet_build_graph, the cell list leaves out pairs of two weight-0 atoms (nothing of a
 * ghost's own neighbourhood is used).  If the weight-1 atoms are one contiguous range of the engine's cell order (cells are numbered
 * x-major; a slab along x whose faces are cell faces of tmdnet_set_cell_grid's grid is such a range), the per-atom kernels and the
 * forward sweeps run on that range only: tmdnet_get_info "halo_active_first" / "halo_active_rows" report it. */
typedef int (*tmdnet_halo_exchange_fn)(void* user, int32_t stage, float* rows, int64_t n_rows, int64_t row_floats,
                                       const int32_t* perm, void* stream);
int tmdnet_set_halo_exchange(tmdnet_model* m, tmdnet_halo_exchange_fn fn, void* user);
int tmdnet_build_graph(tmdnet_model* m, void* stream, void* graph_ws, size_t graph_ws_bytes, int64_t n_atoms, int64_t n_mol,
                       const float* pos, const int64_t* batch, const int64_t* z, const float* box, int32_t box_mode,
                       int64_t counts_host[8]);

/* Static (HIP-graph capturable) variant: same kernels, NO read-back and no synchronisation.  The pair count
 * stays in device memory; call tmdnet_energy_forces with n_pairs = -1 and workspaces sized for the pair
 * capacity (tmdnet_forward_workspace_bytes with n_pairs = -1).  On overflow the kernels of both phases skip
 * their work (outputs undefined) and the flag is left in the graph workspace: poll it with
 * tmdnet_graph_counts (synchronises; returns TMDNET_ERR_OVERFLOW) whenever convenient -- the analogue of the
 * reference's torch._assert_async (torchmdnet/models/utils.py:297-300). */
int tmdnet_build_graph_static(tmdnet_model* m, void* stream, void* graph_ws, size_t graph_ws_bytes, int64_t n_atoms,
                              int64_t n_mol, const float* pos, const int64_t* batch, const int64_t* z, const float* box,
                              int32_t box_mode);
/* out-of-range z / batch (flags [4], [5]) return TMDNET_ERR_INVALID here; in static mode the kernels ran on clamped
 * atomic numbers (memory-safe, results meaningless) */
int tmdnet_graph_counts(tmdnet_model* m, void* stream, void* graph_ws, int64_t n_atoms, int64_t n_mol, int64_t counts_host[8]);
/* cell grid of the last build on this workspace (synchronises): grid_host = {n_x, n_y, n_z, 1 if the cell list ran else 0} */
int tmdnet_graph_cell_grid(tmdnet_model* m, void* stream, void* graph_ws, int64_t n_atoms, int64_t n_mol, int64_t grid_host[4]);

/* ---- phase B: energies and forces ---------------------------------------------------------------
 * Replaces TorchMD_Net.forward for TensorNet + Scalar (torchmdnet/models/model.py:530-631):
 * energy[n_mol] = sum over atoms of the per-atom scalar (* std, + atomref[z]) + mean, and
 * forces[n_atoms,3] = -d(sum_m energy[m])/d(pos) from the hand-written reverse pass
 * (want_forces = 0 skips it).  `q` = total charge per molecule [n_mol] or NULL (tensornet.py:341-344).
 * `z` may be NULL when tmdnet_build_graph[_static] received (and validated) it.
 * Must be called after tmdnet_build_graph on the same graph_ws (which holds the pair geometry);
 * n_pairs = counts_host[0] of that call (or -1 after tmdnet_build_graph_static).  Enqueues only: no
 * synchronisation, no allocation.  The handle remembers per graph_ws address what it was last built as (cell list or
 * not, validated z, species count): builds on several workspaces may be interleaved with their evaluations.
 * tmdnet_forward_workspace_bytes does not depend on which build came last (the species-dependent buffers are sized for
 * their largest padding). */
int tmdnet_forward_workspace_bytes(const tmdnet_model* m, int64_t n_atoms, int64_t n_mol, int64_t n_pairs, int64_t n_edges,
                                   int32_t want_forces, size_t* bytes);
int tmdnet_energy_forces(tmdnet_model* m, void* stream, void* graph_ws, void* ws, size_t ws_bytes, int64_t n_atoms,
                         int64_t n_mol, int64_t n_pairs, const int64_t* z, const int64_t* batch, const float* q,
                         int32_t want_forces, float* energy, float* forces);

/* The same call that also returns the virial of every molecule (TensorNet and Equivariant Transformer handles, scalar head; the
 * reference has no counterpart).  Definition, with row vectors: under the homogeneous strain pos -> pos (I + eps), box -> box (I + eps),
 * one eps[3,3] per molecule,
 *     W_m[a][b] = - d E_m / d eps_ab |_(eps = 0) = - sum over the pairs p of molecule m of  delta_p[a] * (d E / d delta_p)[b]
 * with delta_p = pos_i - pos_j (+ minimum image) as the graph phase stored it: the box scales with the positions, so every pair keeps
 * its image and the pair form is exact.  Self pairs contribute nothing; mean, std and atomref enter as they enter the forces.  Sign:
 * W is MINUS the strain derivative (for a pair potential, W = sum_p delta_p (x) f_p with f_p the force on the pair's i end), and the
 * stress of molecule m in a cell of volume V_m = |det box_m| is  sigma_m = - W_m / V_m.  `virial` is device memory, [n_mol][9],
 * row-major a * 3 + b, the full tensor: it is NOT symmetrised (it is symmetric up to rounding because the energy is rotation
 * invariant; the tests check that).  A molecule index without atoms gets zeros.
 * Arguments as tmdnet_energy_forces (want_forces is accepted for symmetry and ignored: the virial is a by-product of the force pass,
 * the call behaves as if it were 1; `forces` is required) plus the scratch `virial_ws` of tmdnet_virial_workspace_bytes(n_atoms, n_mol)
 * bytes (device; 36 bytes per atom plus the slice sums of large molecules).  `energy` and `forces` are bit-identical to those
 * tmdnet_energy_forces writes for the same inputs; the virial is reduced in a fixed order without atomics (bit-identical repeats).
 * Enqueues only: no allocation, no synchronisation, capturable (static mode: skipped on overflow like the rest of the step).
 * TMDNET_ERR_INVALID for a TensorNet2 handle (its Coulomb forces do not come from the per-pair gradient), a property head
 * (tmdnet_set_output_head), atom weights or a halo exchange set, or inside the parameter-gradient / second-order passes. */
int tmdnet_virial_workspace_bytes(const tmdnet_model* m, int64_t n_atoms, int64_t n_mol, size_t* bytes);
int tmdnet_energy_forces_virial(tmdnet_model* m, void* stream, void* graph_ws, void* ws, size_t ws_bytes, void* virial_ws,
                                size_t virial_ws_bytes, int64_t n_atoms, int64_t n_mol, int64_t n_pairs, const int64_t* z,
                                const int64_t* batch, const float* q, int32_t want_forces, float* energy, float* forces, float* virial);

/* ---- fine-grained operator: the reference's neighbour op --------------------------------------
 * Same outputs as torch.ops.torchmdnet.warp_neighbor_brute_fwd (warp_ops/neighbors.py:34-148):
 * neighbors int64 [2,max_num_pairs] padded with -1, deltas [max_num_pairs,3], distances
 * [max_num_pairs], num_pairs int32[1] (the true count, may exceed max_num_pairs).  Pair order is
 * deterministic: lower pairs (i>j) sorted by (i,j), then their transposes, then self loops.
 * strategy 0 = brute force inside each molecule; 1 = O(N) cell list (tn_cell.hip) over all molecules at once, pairs kept
 * inside a molecule: one periodic box (box_mode 1) or, without a box, a fictitious one around the bounding box of the
 * positions (the reference: models/utils.py:206-212); per-molecule boxes (box_mode 2) always take strategy 0.  Same
 * pair set either way (order differs: cell order).
 * `ws` must hold tmdnet_neighbor_workspace_bytes(n_atoms, n_mol, max_num_pairs). */
int tmdnet_neighbor_workspace_bytes(int64_t n_atoms, int64_t n_mol, int64_t max_num_pairs, size_t* bytes);
int tmdnet_neighbor_pairs(void* stream, void* ws, size_t ws_bytes, int64_t n_atoms, int64_t n_mol, const float* pos,
                          const int64_t* batch, const float* box, int32_t box_mode, float cutoff_lower, float cutoff_upper,
                          int64_t max_num_pairs, int32_t loop, int32_t include_transpose, int32_t strategy, int64_t* neighbors,
                          float* deltas, float* distances, int32_t* num_pairs);

/* Gradient of (deltas, distances) wrt the positions: the reference's neighbor_grad_positions
 * (torchmdnet/extensions/neighbor_utils.py:11-46), registered as the backward of its neighbour ops
 * (warp_ops/neighbors.py:105-148).  neighbors int64 [2, num_entries] (padding -1 is skipped, d = 0 contributes nothing),
 * grad_deltas [num_entries,3] / grad_distances [num_entries] may be NULL (= zero); grad_positions [n_atoms,3] is overwritten. */
int tmdnet_neighbor_grad(void* stream, const int64_t* neighbors, const float* deltas, const float* distances,
                         const float* grad_deltas, const float* grad_distances, int64_t num_entries, int64_t n_atoms,
                         float* grad_positions);

/* The same operator for DOUBLE positions (ABI 9).  The reference's neighbour kernels are generic over the position dtype
 * (torchmdnet/extensions/warp_kernels/neighbors_brute.py:27-175 and neighbors_cell.py:17-153 are instantiated for float32 and
 * float64; torchmdnet/extensions/warp_ops/neighbors.py:34-148 dispatches on positions.dtype; tests/test_neighbors.py:83,157,281
 * run both).  Outputs, padding, overflow reporting and the order (lower pairs by (i, j), their transposes, self loops) as above;
 * every strategy takes the brute-force search (same pair set); `ws` as for tmdnet_neighbor_pairs.  The model path stays fp32. */
int tmdnet_neighbor_pairs_f64(void* stream, void* ws, size_t ws_bytes, int64_t n_atoms, int64_t n_mol, const double* pos,
                              const int64_t* batch, const double* box, int32_t box_mode, double cutoff_lower, double cutoff_upper,
                              int64_t max_num_pairs, int32_t loop, int32_t include_transpose, int64_t* neighbors, double* deltas,
                              double* distances, int32_t* num_pairs);
int tmdnet_neighbor_grad_f64(void* stream, const int64_t* neighbors, const double* deltas, const double* distances,
                             const double* grad_deltas, const double* grad_distances, int64_t num_entries, int64_t n_atoms,
                             double* grad_positions);

/* ---- per-kernel-class timing (HIP events recorded on the launch stream around every launch of the
 * selected classes; bit c of category_mask selects class c).  tmdnet_profile_end synchronises the
 * stream and returns, per class: summed milliseconds, algorithmic FLOPs, algorithmic bytes (each distinct
 * input/output tensor of a launch counted once) and the number of launches.
 * Arrays must hold tmdnet_profile_num_categories() entries.  Used by bench.py for `roofline`. */
int tmdnet_profile_begin(tmdnet_model* m, uint32_t category_mask);
int tmdnet_profile_end(tmdnet_model* m, void* stream, double* ms, double* flops, double* bytes, int64_t* launches);
/* the same per launch, in launch order (up to `cap` records are written, *n_out = number recorded); `labels` (may be
 * NULL) receives one 64-byte NUL-terminated string per record naming the launch (kernel wrapper + shape): bench.py groups
 * by it to single out the dominant KERNEL of a class */
int tmdnet_profile_end_records(tmdnet_model* m, void* stream, int64_t cap, int32_t* cat, double* ms, double* flops, double* bytes,
                               char* labels, int64_t* n_out);
int tmdnet_profile_num_categories(void);
const char* tmdnet_profile_category_name(int idx);

/* ---- diagnostics ---------------------------------------------------------------------------------
 * Copy an intermediate of the last tmdnet_energy_forces call out of the workspace (device -> device).
 * Names: "X_embed", "X_layer<l>", "x", "phi", "Q", "u0", "G_embed".  Used by the parity tests. */
int tmdnet_debug_tensor(tmdnet_model* m, void* stream, const char* name, float* out, int64_t numel);
/* Copy one array of the graph that tmdnet_build_graph[_static] last left in `graph_ws` into the device buffer `out` (device ->
 * device on `stream`, no kernel; n_atoms / n_mol as in that build, `bytes` = the array's whole capacity).  Names, element type
 * and count, with ecap = max_num_neighbors * n_atoms and pcap = ecap / 2 + 1: int32 "counts" [8], "mstart" / "mend" [n_mol],
 * "nlow" / "ntot" / "perm" / "cell_key_sorted" [n_atoms], "rowptr" / "pairptr" [n_atoms + 1], "col" / "epair" [ecap],
 * "pair_i" / "pair_j" [pcap], "cgrid" [4], "cell_start" [8 n_atoms + 2]; float "esign" [ecap], "pd" [pcap + 1],
 * "pdelta" / "prhat" [3 pcap], "boxd" [12]; int64 "z_c" / "bat_c" [n_atoms].  TMDNET_ERR_STATE when no graph was built on
 * `graph_ws`, TMDNET_ERR_INVALID for an unknown name, a wrong byte count or other n_atoms / n_mol; nothing is written then.
 * Used by the graph unit tests (tests/test_gpu_graph.py). */
int tmdnet_debug_graph(tmdnet_model* m, void* stream, const void* graph_ws, int64_t n_atoms, int64_t n_mol, const char* name,
                       void* out, int64_t bytes);
/* plain dense contraction through the path's MFMA GEMM: C[M,N] = A[M,K] @ W[N,K]^T (+bias) (silu != 0: silu of it); Wsb as
 * for tmdnet_debug_gemm_dual (NULL: fp32-MFMA kernels); for unit tests */
/* value + tangent GEMM of the edge MLP (kind 0 plain, 1 silu, 2 silu * rs with rs2 = d rs): C = f(A W^T + b), C2 = d/dd.
 * Wsb: optional DEVICE copy of the split-bf16 tile image of W (tmdnet_debug_split_weight); when given and the shape
 * qualifies, the bf16-MFMA kernel runs instead of the fp32-MFMA one. */
int tmdnet_debug_gemm_dual(void* stream, const float* A, const float* A2, const float* W, const float* bias, float* C, float* C2,
                           int64_t M, int64_t N, int64_t K, int32_t kind, const float* rs, const float* rs2, const uint16_t* Wsb);
/* host-side 3 x bf16 split of W[N,K] into the kernel's tile image; returns the number of uint16 elements
 * (out_host may be NULL to query the size) */
int64_t tmdnet_debug_split_weight(const float* W_host, int64_t N, int64_t K, uint16_t* out_host);
int tmdnet_debug_gemm(void* stream, const float* A, const float* W, const float* bias, float* C, int64_t M, int64_t N,
                      int64_t K, int32_t silu, const uint16_t* Wsb);
/* (The two entries below are additive: no existing signature or struct changed, the ABI revision stays.)
 * The single-product GEMM family behind every dense contraction (fp32-MFMA tiles, split-K, split-bf16), with the whole
 * argument surface the schedules use: epilogue flags, up to nine groups with per-group offsets, leading dimensions and the
 * device-side row count.  No model handle; for unit tests.
 *   C[g][m, n] = epilogue( sum_k A[g][m, k] W[g][n, k] + bias[g][n] ),  A[g] = A + a_off[g] (likewise C / pre / aux), g < groups
 *   flags (TMDNET_GEMM_*), applied in this order: pre[m, n] = value (when pre != NULL); silu; * rowscale[m]; * aux[m, n];
 *   * silu'(aux[m, n]); + old C[m, n].  Rows: min(M, *m_dev + m_add) when m_dev != NULL (a DEVICE int), else M; rows past that
 *   count are not written.  Wsbg[g]: DEVICE copy of the split-bf16 tile image of W[g] (tmdnet_debug_split_weight) or NULL; when
 *   every group has one and the shape qualifies a split-bf16 kernel runs.
 * *route_out (may be NULL) receives the kernel taken, one of TMDNET_GEMM_ROUTE_*: the value of the selection function the
 * launchers themselves branch on, not a second copy of their thresholds (those are performance choices and may move).
 * TMDNET_ERR_INVALID, and no launch, outside the kernels' contract: N < 1, K < 1, M < 0, groups outside 1..9, unknown flag bits,
 * NULL A / C / W[g], NULL rowscale or aux when a flag reads it, a leading dimension shorter than its row, a negative offset. */
#define TMDNET_GEMM_MAX_GROUPS 9
#define TMDNET_GEMM_ACT_SILU 1
#define TMDNET_GEMM_MUL_AUX 2
#define TMDNET_GEMM_MUL_DSILU_AUX 4
#define TMDNET_GEMM_ACCUM 8
#define TMDNET_GEMM_ROWSCALE 16
#define TMDNET_GEMM_ROUTE_NONE 0          /* M == 0: nothing launched */
#define TMDNET_GEMM_ROUTE_SKINNY4 1       /* split-K over 4 waves, 32 x 32 outputs per block (K < 256) */
#define TMDNET_GEMM_ROUTE_SKINNY8 2       /* split-K over 8 waves (K >= 256) */
#define TMDNET_GEMM_ROUTE_TILES_128X128 3 /* fp32-MFMA tiles */
#define TMDNET_GEMM_ROUTE_TILES_128X64 4
#define TMDNET_GEMM_ROUTE_TILES_128X32 5
#define TMDNET_GEMM_ROUTE_SB1_128 6       /* split-bf16, persistent 128 x 128 tiles */
#define TMDNET_GEMM_ROUTE_SB1_64 7        /* split-bf16, 64 x 64 tiles (fewer 128-tiles than compute units) */
typedef struct tmdnet_gemm_ex_args {
  const float* A;
  const float* W[TMDNET_GEMM_MAX_GROUPS];
  const float* bias[TMDNET_GEMM_MAX_GROUPS]; /* [N] or NULL */
  float* C;
  float* pre;            /* optional */
  const float* aux;      /* operand of MUL_AUX / MUL_DSILU_AUX */
  const float* rowscale; /* [M], operand of ROWSCALE */
  int64_t lda, ldw, ldc, ldpre, ldaux;
  int32_t a_off[TMDNET_GEMM_MAX_GROUPS], c_off[TMDNET_GEMM_MAX_GROUPS], pre_off[TMDNET_GEMM_MAX_GROUPS],
      aux_off[TMDNET_GEMM_MAX_GROUPS];
  int32_t M, N, K, groups, flags;
  const int32_t* m_dev; /* DEVICE row count or NULL */
  int32_t m_add;
  const uint16_t* Wsbg[TMDNET_GEMM_MAX_GROUPS];
} tmdnet_gemm_ex_args;
int tmdnet_debug_gemm_ex(void* stream, const tmdnet_gemm_ex_args* args, int32_t* route_out);
/* One launch of the fused nine-component tensor linear (the kernel of every per-atom tensor contraction at batch scale):
 *   C[atom, c, n] = epilogue( sum_k prologue(A)[atom, c, k] W_type(c)[n, k] ),  type(c) = 0 (c = 0) | 1 (c = 1..3) | 2 (c = 4..8)
 * pro: 0 plain, 1 A / (quad(A) + 1), 2 update adjoint of (A, A2, kap).  epi: 0 plain, 1 gate multiply (e3 = gates [N, 3, F],
 * o1 = product before the gates), 2 update (e0 = X; o1 = new X; o2 = its invariants [N, 3, F] when want_feat), 3 normalisation
 * adjoint (e0 = X, e1 = incoming gradient; C may alias e1), 4 the same followed by the gate adjoint (e2 = UX, e3 = gates,
 * e4 = gate pre-activations [N, 3, F]; o1 = their gradient [N, 3, F]), 5 embedding atom adjoint (e0 = X, e1 = [N, F];
 * o1 = [N, 10, F]; C is not written).  The launched pairs are (0,0) (1,0) (2,0) and (0,1..5).  All tensors [N, 9, F] fp32 unless
 * noted; kap [N] or NULL (= 1); W_I / W_A / W_S are DEVICE fp32 [F, F] matrices.  No model handle; for unit tests.
 * scratch: DEVICE memory for the three fragment-major split-bf16 weight images, built here on `stream` before the launch.
 * With scratch == NULL the call only writes the needed number of uint16 elements to *scratch_elems; otherwise *scratch_elems
 * is the number provided.  The row-count rule of the model's schedule (at least 128 tiles of 32 atoms x 128 channels) is a
 * performance threshold and is NOT applied here: the kernel clamps the rows of a partial tile itself, so any N >= 1 runs.
 * TMDNET_ERR_INVALID, and no launch, outside the kernel's contract: F % 128 != 0, N < 1, a (pro, epi) pair that is not
 * launched, a NULL or misaligned (8 bytes) operand the pair reads or writes, a scratch that is too small. */
int tmdnet_debug_tlin9(void* stream, int32_t pro, int32_t epi, int64_t N, int64_t F, const float* A, const float* A2, float* C,
                       const float* e0, const float* e1, const float* e2, const float* e3, const float* e4, float* o1, float* o2,
                       const float* kap, int32_t want_feat, const float* W_I, const float* W_A, const float* W_S,
                       uint16_t* scratch, int64_t* scratch_elems);
/* One launch of a TensorNet neighbour sweep on a caller-built graph (additive as well: the ABI revision stays).  No model
 * handle; for unit tests.  The sweeps (type(c) as above, p = epair[e], j = col[e], e over rowptr[i] .. rowptr[i + 1]):
 *   TMDNET_MSG_OP_FWD   out[i, c, f] = M = sum_e w[p, type(c), f] src[j, c, f];  out2 = dec(C) / (quad(C) + 1) with
 *                       C = kap (Y M + M Y) (o3 != 0) or 2 Y M, Y = src[i], kap = 1 + 0.1 q[batch[i]] (batch != NULL), q[i]
 *                       (batch == NULL) or 1 (q == NULL)
 *   TMDNET_MSG_OP_ADJ   out[i] += sum_e w[p] src[j]
 *   TMDNET_MSG_OP_GD    the same, and slots[a][2 p + dir] = sum over the channels of group a of w2[p, k, f] sum_{c in k}
 *                       src[j, c, f] src2[i, c, f]  (w2 = dw, src = gMi, src2 = Pn; dir 0: row i is the pair's first atom, j < i)
 *   TMDNET_MSG_OP_DUAL  out[i] (+)= sum_e w[p] src[j];  out2[i] (+)= sum_e w[p] src2[j] + sum_e w2[p] src[j]  (w2 = w_t, src2 = src_t)
 * w, w2: [P + 1, 3, F]; src, src2, out, out2: [N, 9, F]; slots: arrays of slot_stride >= 2 P floats; all fp32, DEVICE memory.
 * The graph must be in the engine's own form and is NOT validated here: rowptr [N + 1], col / epair / esign per entry, the
 * adjacency symmetric, the columns of a row ascending, a self edge with pair id P in every row, esign +1 where the row atom is
 * the pair's first atom (col < row), -1 where it is the second, 0 on the self edge; counts [8] as the engine keeps them
 * (counts[2] != 0: pair overflow, every kernel returns without writing).  Anything else reads or writes out of bounds.
 * kernel: TMDNET_MSG_AUTO calls the sweep's launcher with (N, F, small_mols) (and `accumulate` for OP_DUAL); any other value
 * launches that kernel itself - the launchers' size thresholds are performance choices and are not applied.  *route_out (may be
 * NULL) receives the kernel taken: the value of the selection function the launcher switches on (a model handle reports the
 * routes of its last energy / force call the same way: tmdnet_get_info "message_route_last", "message_adjoint_route_last").
 * Both out-parameters are written only when the call launches (TMDNET_OK, or TMDNET_ERR_HIP from the launch itself).  *slot_arrays_out (may be
 * NULL) receives the number of slot arrays the kernel writes: F / 64 (row and split kernels), F / 32 (tile kernel), 0 without
 * slots.  balance (forward tile kernel): 0 every row walked by its own lanes, 1 long rows hand their tails to short ones, < 0 default.
 * TMDNET_ERR_INVALID, and no launch, outside the selected kernel's contract: N < 1, F < 1, P < 0, a kernel of another sweep or
 * an unknown one, F % 32 (tile kernels; their operands 16-byte aligned), F % 64 or F > 128 (split kernels), F % 64 or F > 1024
 * (TMDNET_MSG_GD_ROW), slot_stride < 2 P, a NULL graph array or a NULL operand the kernel reads or writes. */
#define TMDNET_MSG_OP_FWD 0
#define TMDNET_MSG_OP_ADJ 1
#define TMDNET_MSG_OP_GD 2
#define TMDNET_MSG_OP_DUAL 3
#define TMDNET_MSG_AUTO 0
#define TMDNET_MSG_FWD_ROW 1    /* k_message<false> */
#define TMDNET_MSG_FWD_SPLIT 2  /* k_message_split<0> */
#define TMDNET_MSG_FWD_TILE 3   /* k_message_rows8<8, 4> */
#define TMDNET_MSG_ADJ_ROW 4    /* k_message_adjoint */
#define TMDNET_MSG_ADJ_SPLIT 5  /* k_message_split<1> */
#define TMDNET_MSG_GD_ROW 6     /* k_message_adjoint_gd<false> */
#define TMDNET_MSG_GD_SPLIT 7   /* k_message_split<2> */
#define TMDNET_MSG_GD_TILE 8    /* k_message_adjoint_rows8 */
#define TMDNET_MSG_DUAL 9       /* k_message_dual<false>: out = ... */
#define TMDNET_MSG_DUAL_ACC 10  /* k_message_dual<true>: out += ... */
#define TMDNET_MSG_DUAL_SPLIT3 16 /* route of TMDNET_MSG_AUTO only: three k_message_split<1> launches */
typedef struct tmdnet_message_args {
  int32_t op, kernel;
  int32_t N, F, P, small_mols, o3, balance, accumulate;
  const int32_t* rowptr; /* [N + 1] */
  const int32_t* col;
  const int32_t* epair;
  const float* esign;
  const int32_t* counts; /* [8] */
  const float* w;
  const float* w2;   /* dw (OP_GD) or w_t (OP_DUAL) */
  const float* src;  /* src (OP_FWD, OP_DUAL) or gMi (OP_ADJ, OP_GD) */
  const float* src2; /* Pn (OP_GD) or src_t (OP_DUAL) */
  const float* q;    /* OP_FWD, optional */
  const int64_t* batch; /* OP_FWD, optional */
  float* out;  /* Mi (OP_FWD), gPn (OP_ADJ, OP_GD), out (OP_DUAL) */
  float* out2; /* Ch (OP_FWD), out_t (OP_DUAL) */
  float* slots;
  int64_t slot_stride;
} tmdnet_message_args;
int tmdnet_debug_message(void* stream, const tmdnet_message_args* args, int32_t* route_out, int32_t* slot_arrays_out);
/* The reverse tile sweep with the adjoint of the group product in its prologue (k_message_adjoint_rows8_fold), or the sequence it
 * replaces, on a caller-built graph (additive; no model handle; for unit tests).  With gM, gY the gradients of
 * sum(gCh * C_hat(Pn, Mi)) with respect to Mi and Pn (C_hat as out2 of TMDNET_MSG_OP_FWD above, kap from q / batch the same way):
 *   gPn[i] = gY[i] + sum_e w[p] gM[j];   slots[a][2 p + dir] as TMDNET_MSG_OP_GD above with src = gM, src2 = Pn, a over F / 32.
 * folded != 0: one launch; gMi is neither read nor written (may be NULL).  folded == 0: k_message_bwd_node writes gMi and gY,
 * then k_message_adjoint_rows8 - the same result, gMi required.  gPn need not be initialised in either mode.
 * The graph is in the engine's form (tmdnet_debug_message) and, for folded != 0, must have CLOSED tiles: col[e] / 64 == i / 64
 * for every entry e of every row i.  This one property IS validated (the arrays are read back; the call synchronises the
 * stream): TMDNET_ERR_INVALID and no launch otherwise, as for N < 1, P < 0, F % 32, slot_stride < 2 P, a NULL or misaligned
 * (16 bytes) operand. */
typedef struct tmdnet_message_fold_args {
  int32_t N, F, P, o3, folded;
  const int32_t* rowptr; /* [N + 1] */
  const int32_t* col;
  const int32_t* epair;
  const float* esign;
  const int32_t* counts; /* [8] */
  const float* w;        /* [P + 1, 3, F] */
  const float* dw;       /* [P + 1, 3, F] */
  const float* gCh;      /* [N, 9, F] */
  const float* Pn;       /* [N, 9, F] */
  const float* Mi;       /* [N, 9, F] */
  const float* q;        /* optional */
  const int64_t* batch;  /* optional */
  float* gMi;            /* [N, 9, F], written when folded == 0 */
  float* gPn;            /* [N, 9, F] */
  float* slots;          /* F / 32 arrays of slot_stride floats */
  int64_t slot_stride;
} tmdnet_message_fold_args;
int tmdnet_debug_message_fold(void* stream, const tmdnet_message_fold_args* args);
/* One launch of a kernel only the TensorNet2 + ScalarPlusWeightedCoulomb path has (csrc/tn_tn2.hip), through its own launcher, on
 * caller-built operands (additive as well: the ABI revision stays).  No model handle; for unit tests.  The graph is in the
 * engine's form (tmdnet_debug_message) and is NOT validated: rowptr [N + 1], col / epair per entry (E = rowptr[N] entries), the
 * adjacency symmetric, the columns of a row ascending, a self edge with pair id P in every row; counts [8] as the engine keeps
 * them (counts[0] = P; counts[2] != 0: pair overflow, the edge kernels return without writing; counts[3] != 0: `batch` is not
 * sorted, the per-molecule kernels scan all atoms and filter by `batch` instead of walking mstart[m] .. mend[m]); mstart / mend
 * [B].  All float operands fp32, DEVICE memory.  With e = (i <- j) an entry of row i, j = col[e], p = epair[e], r the entry
 * (j <- i), rows [.., 3 F] as [.., 3, F], type(c) = 0 (c = 0) | 1 (c = 1..3) | 2 (c = 4..8):
 *   EDGE_REVERSE  erev[e] = r, eid[e] = e  [E];  pair_edge[p] = the entry with j < i of pair p  [P]
 *   CP_FEAT       feat [N, 3, F] = [I ; |A|^2 ; |S|^2] of X [N, 9, F] (I = component 0)
 *   CP_FEAT_BWD   G [N, 9, F] += (d feat / d X)^T g_feat
 *   QEQ_FWD       out [N, 2 qd] = [r | f]:  Fu = sum_mol f^2 + 1e-6, dQ = Qmol[m] - sum_mol r (Qmol NULL: 0),
 *                 charges [N, qd] = r + f^2 / Fu dQ,  FuQ [B, 2 qd] = [Fu | dQ]
 *   QEQ_BWD       g_out [N, 2 qd] = [g_c - S1 | 2 f dQ / Fu (g_c - S1)],  S1 = sum_mol g_c f^2 / Fu   (Fu, dQ read from FuQ)
 *   EDGE_PRE1     pre1 [E, F] = Ap[p] + Bt[i] + Cs[j], he1 = silu(pre1), Ce [E] = C[p]   (Ap [P + 1, F], C [P + 1], Bt / Cs [N, F])
 *   EDGE_GW       g_w[e, k, f] = sum_{type(c) = k} gMi[i, c, f] Pn[j, c, f];  g_pre3 [E, 3 F] = g_w Ce[e] silu'(pre3);
 *                 slots[a][e] = sum over k and the channels 64 a .. 64 a + 63 of g_w silu(pre3), a < *slot_arrays_out
 *   EDGE_REDUCE   gB[i] = sum_{e in row i} g_pre1[e], gCs[i] = sum_{e in row i} g_pre1[r]  [N, F];  gAp[p] = g_pre1[e] + g_pre1[r]
 *                 for the entry with j < i of pair p  [P, F] (rows of no such entry are not written)
 *   PAIR_GD       gd[p] += sum_f gAp[p, f] dAp[p, f] + dC[p] sum_a (slots[a][e] + slots[a][r]), e = pair_edge[p], p < counts[0], p < P
 *   COULOMB       ec[i] = sum_j F0 fc(d) g(d) sum_k wq[k] q[i, k] q[j, k] / sum_k wq[k] over the atoms j != i with batch[j] ==
 *                 batch[i] (batch NULL: one molecule) and, for cut > 0, d < cut;  F0 = 7.199822675975274, fc = 1 - exp(1 -
 *                 1 / (1 - u^2)), u = min(d / 4.6, 1 - 1e-6);  g = 1 / d (cut <= 0) or 1 / d + k_rf d^2 - c_rf (reaction field of
 *                 eps_solvent);  d with the triclinic minimum image (z, y, x in turn) of `box` [3, 3] (box_mode 1) or
 *                 box[batch[i]] (box_mode 2), none for box_mode 0;  an atom with batch outside 0 .. B - 1 gets ec = 0.
 *                 With g_q != NULL also g_q [N, QC] = d (scale sum ec) / d q and fpos [N, 3] = - d (scale sum ec) / d pos.
 * *slot_arrays_out (may be NULL) receives the number of slot arrays of EDGE_GW / PAIR_GD for this F (every op writes it when the
 * call launches); every array has slot_stride >= E floats.
 * TMDNET_ERR_INVALID, and no launch, outside the kernel's contract: an unknown op, N < 1, B < 1 (QEQ, COULOMB), P < 0, E < 0,
 * F < 1 (the ops with channels), F > 1024 (EDGE_GW), qd < 1 or qd > 256 (QEQ), QC < 1 or QC > 64 (COULOMB), box_mode outside
 * 0 .. 2 or without a box, fpos NULL with g_q given, slot_stride < E (EDGE_GW, PAIR_GD), a NULL graph array or operand the op
 * reads or writes (Qmol, batch of COULOMB, g_q and fpos are optional). */
#define TMDNET_TN2_EDGE_REVERSE 0
#define TMDNET_TN2_CP_FEAT 1
#define TMDNET_TN2_CP_FEAT_BWD 2
#define TMDNET_TN2_QEQ_FWD 3
#define TMDNET_TN2_QEQ_BWD 4
#define TMDNET_TN2_EDGE_PRE1 5
#define TMDNET_TN2_EDGE_GW 6
#define TMDNET_TN2_EDGE_REDUCE 7
#define TMDNET_TN2_PAIR_GD 8
#define TMDNET_TN2_COULOMB 9
typedef struct tmdnet_tn2_unit_args {
  int32_t op;
  int32_t N, B, F, P, E, qd, QC, box_mode;
  float cut, eps_solvent, scale;
  int64_t slot_stride;
  int32_t* slot_arrays_out; /* HOST, optional */
  /* graph */
  const int32_t* rowptr; /* [N + 1] */
  const int32_t* col;
  const int32_t* epair;
  const int32_t* counts; /* [8] */
  const int32_t* mstart; /* [B] */
  const int32_t* mend;   /* [B] */
  const int64_t* batch;  /* [N] */
  /* EDGE_REVERSE writes these; EDGE_REDUCE reads erev, PAIR_GD reads erev and pair_edge */
  int32_t* erev;
  int32_t* eid;
  int32_t* pair_edge;
  /* CP_FEAT, CP_FEAT_BWD */
  const float* X;
  const float* g_feat;
  float* feat;
  float* G;
  /* QEQ_FWD, QEQ_BWD (FuQ: written by FWD, read by BWD) */
  const float* out;
  const float* Qmol;
  const float* g_c;
  float* charges; /* QEQ_FWD output; COULOMB input [N, QC] */
  float* FuQ;
  float* g_out;
  /* EDGE_PRE1 (Ce: written here, read by EDGE_GW) */
  const float* Ap;
  const float* Bt;
  const float* Cs;
  const float* C;
  float* pre1;
  float* he1;
  float* Ce;
  /* EDGE_GW (slots: written here, read by PAIR_GD) */
  const float* gMi;
  const float* Pn;
  const float* pre3;
  float* g_pre3;
  float* slots;
  /* EDGE_REDUCE (gAp: written here, read by PAIR_GD) */
  const float* g_pre1;
  float* gB;
  float* gCs;
  float* gAp;
  /* PAIR_GD */
  const float* dAp;
  const float* dC;
  float* gd;
  /* COULOMB */
  const float* pos;
  const float* box;
  const float* wq;
  float* ec;
  float* g_q;
  float* fpos;
} tmdnet_tn2_unit_args;
int tmdnet_debug_tn2(void* stream, const tmdnet_tn2_unit_args* args);
/* One kernel of the Equivariant Transformer's edge sweeps (csrc/tn_et.hip, csrc/tn_et_g16.hip) on caller-built operands
 * (additive: the ABI revision stays).  No model handle; for unit tests.  The graph is in the engine's form (tmdnet_debug_message)
 * and is NOT validated; beyond the CSR it has pair_i / pair_j [P] (pair_i > pair_j), prhat [P, 3] = the unit vector of
 * pos[pair_i] - pos[pair_j], and `batch` [N] (sorted; NULL: one molecule).  counts[0] = P, counts[1] = E = rowptr[N].
 * Layouts: qkv [N, 5 F] = q | k | vx | v1 | v2; vec, vagg, g_vagg, g_vec [N, 3, F]; xagg, g_xagg [N, F]; C, dC [P + 1]; dkv, tkv
 * [P + 1, Wd] with the key projection's F columns at dk_off and the value projection's 3 F at dv_off (-1: the model has no such
 * projection, the factor is 1 and its tangent 0; both -1: dkv and tkv may be NULL), fp32, or bf16 when pair_bf16 = 1.  Channel c
 * belongs to head c / hd.  With e = (i <- j) an entry of row i, p = epair[e], rhat = -esign[e] prhat[p] (0 on the self edge),
 * cv = C[p], ca = 1 (vector_cutoff != 0) or cv = 1, ca = C[p]:
 *   a[e, h] = sum_{c in h} q[i, c] k[j, c] dk[p, c];  A = silu(a) ca;  sx = vx[j] cv dvx[p], s1 = v1[j] cv dv1[p], s2 = v2[j] cv dv2[p]
 *   TMDNET_ET_OP_ATTN_FWD      xagg[i] = sum_e sx A;  vagg[i, x] = sum_e vec[j, x] s1 + s2 rhat_x
 *   TMDNET_ET_OP_ATTN_BWD      the adjoint for given g_xagg, g_vagg: g_qkv [N, 5 F] written, g_vec [N, 3, F] +=, and per slot
 *                              array w the partial sums over its channels of d / d d(p) and d / d rhat of the edge (i <- j), at
 *                              gd2[w slot_stride + 2 p + dir], gr2[(w slot_stride + 2 p + dir) 3 + x], dir = 0 where esign > 0,
 *                              1 where esign < 0; self edges write no slot.  The caller always sums F / 32 arrays when F % 32 ==
 *                              0 (ceil(F / 64) otherwise): the tile kernels write one per 32 channels, the row kernels one per
 *                              64 and zero the rest.  slot_stride >= 2 (P + 1).
 *   TMDNET_ET_OP_TILE_PREP     meta[0] = 0 when the greedy packing of whole molecules into tiles of at most 64 rows is closed
 *                              and E >= min_fill x tiles x 4096 (else 1), meta[1] = tiles, tile_start [tiles + 1] (array of N + 8),
 *                              erec [E, 8] = col | pair | esign | C | dC | prhat (zeros on the self edge)
 *   TMDNET_ET_OP_PAIR_COMBINE  gd[p] = gd_extra[2 p] + sum_w gd2[w][2 p] + gd2[w][2 p + 1];  g_rhat[p] = sum_w -gr2[w][2 p] +
 *                              gr2[w][2 p + 1]  over nw slot arrays, p < counts[0]
 *   TMDNET_ET_OP_NBR_EMBED     xcat [N, 2 F] = emb[z_i] | sum_{j != i} Wn[p] embN[z_j]
 *   TMDNET_ET_OP_NBR_EMBED_BWD gd2[2 p] += sum_c (g_xcat[i, F + c] embN[z_j, c] + g_xcat[j, F + c] embN[z_i, c]) dWn[p, c]
 *   TMDNET_ET_OP_TRAIN_NBR     slots[dir dir_stride + p F + c] = g_xcat[i, F + c] embN[z_j, c];  gEN[i] = sum_{j != i} g_xcat[j, F +
 *                              c] Wn[p, c]
 *   TMDNET_ET_OP_TRAIN_FILTER  the adjoint of the filter rows dkv per directed edge: slots[dir dir_stride + p Wd + ..] (self
 *                              edges: self_rows [N, Wd]);  g_dk = g_a q_i k_j, g_dvx = cv g_sx vx_j, g_dv1 = cv g_s1 v1_j,
 *                              g_dv2 = cv g_s2 v2_j.  fp32 rows only.
 *   TMDNET_ET_OP_TRAIN_GPRE    g_pre[p] = (slots[p] + slots[dir_stride + p]) silu'(pre[p]), row P from self_sum [Wd]
 *   TMDNET_ET_OP_QUERY         no launch, nothing dereferenced: *route_out = 1 when the tile kernels' size conditions hold for
 *                              (N, P, F, hd, Wd) - 32-bit offsets, and every pair id up to P in the slot table's 24 bits - else 0
 * kernel (the two attention ops): TMDNET_ET_AUTO runs the tile prep and then the engine's own launcher (both generations
 * enqueued, the flag meta[0] on the device picks); TMDNET_ET_ROW_GENERIC k_et_attn_fwd / k_et_attn_bwd; TMDNET_ET_ROW_PIPELINED
 * k_et_attn_fwd_p / k_et_attn_bwd_p (F % 64 == 0, hd <= 16); TMDNET_ET_TILE the prep, then k_et_attn_fwd_g16 / k_et_attn_bwd_g16 alone
 * (TMDNET_ET_OP_QUERY's conditions; it writes nothing when meta[0] != 0).  skip_prep != 0 (AUTO, TILE): meta, tile_start and
 * erec are used as the caller left them.  slot_min, mailbox, sync_every (TILE) and min_fill (TILE_PREP, and the prep of AUTO and
 * TILE) override the developer switches of the tile sweeps; a negative value is the shipped default (slot order from a longest
 * row of 48, mailbox on, 4, 0.70 for fp32 and 0.25 for bf16 rows).  *route_out (may be NULL except for QUERY) receives the
 * generation that wrote the outputs: for AUTO and TILE the call synchronises the stream and reads meta[0] back (TILE with
 * meta[0] != 0: 0, nothing written).
 * TMDNET_ERR_INVALID, and no launch: an unknown op or selector, N < 1, P < 0, B < 1 or E < 0 (ops that run the prep), F < 1, hd
 * no power of two <= 64 or no divisor of F, F > 1024, an offset other than dk_off in {-1, 0}, dv_off in {-1, dk_off + F or 0},
 * Wd smaller than the projections need (odd with bf16 rows), a row kernel outside its F / hd contract, the tile kernel outside
 * QUERY's conditions or with an operand not 16-byte aligned, TRAIN_FILTER with pair_bf16 or without a projection, slot_stride <
 * 2 (P + 1), nw < 1, a NULL graph array or operand the op reads or writes. */
#define TMDNET_ET_OP_QUERY 0
#define TMDNET_ET_OP_TILE_PREP 1
#define TMDNET_ET_OP_ATTN_FWD 2
#define TMDNET_ET_OP_ATTN_BWD 3
#define TMDNET_ET_OP_PAIR_COMBINE 4
#define TMDNET_ET_OP_NBR_EMBED 5
#define TMDNET_ET_OP_NBR_EMBED_BWD 6
#define TMDNET_ET_OP_TRAIN_NBR 7
#define TMDNET_ET_OP_TRAIN_FILTER 8
#define TMDNET_ET_OP_TRAIN_GPRE 9
#define TMDNET_ET_AUTO 0
#define TMDNET_ET_ROW_GENERIC 1
#define TMDNET_ET_ROW_PIPELINED 2
#define TMDNET_ET_TILE 3
typedef struct tmdnet_et_unit_args {
  int32_t op, kernel;
  int32_t N, B, P, E, F, hd, Wd, dk_off, dv_off, vector_cutoff, pair_bf16;
  int32_t skip_prep, slot_min, mailbox, sync_every, nw;
  float min_fill;
  int64_t slot_stride, dir_stride;
  /* graph */
  const int32_t* rowptr; /* [N + 1] */
  const int32_t* col;
  const int32_t* epair;
  const float* esign;
  const int32_t* counts; /* [8] */
  const int32_t* pair_i; /* [P] */
  const int32_t* pair_j;
  const float* prhat;    /* [P, 3] */
  const int64_t* batch;  /* [N], optional */
  /* operands of the attention sweeps */
  const float* C;
  const float* dC;
  const float* qkv;
  const float* vec;
  const void* dkv;
  const void* tkv;
  const float* g_xagg;
  const float* g_vagg;
  /* tile prep (written by TILE_PREP, AUTO and TILE unless skip_prep) */
  int32_t* meta;       /* [2] */
  int32_t* tile_start; /* [N + 8] */
  float* erec;         /* [E, 8] */
  /* outputs of the attention sweeps; gd2 / gr2 are inputs of PAIR_COMBINE, gd2 is the += output of NBR_EMBED_BWD */
  float* xagg;
  float* vagg;
  float* g_qkv;
  float* g_vec;
  float* gd2;
  float* gr2;
  /* PAIR_COMBINE */
  const float* gd_extra; /* [2 (P + 1)] */
  float* gd;             /* [P] */
  float* g_rhat;         /* [P, 3] */
  /* neighbour embedding and its adjoints */
  const int64_t* z;   /* [N] */
  const float* emb;   /* [max_z, F] */
  const float* embN;  /* [max_z, F] */
  const float* Wn;    /* [P + 1, F] */
  const float* dWn;   /* [P + 1, F] */
  const float* g_xcat; /* [N, 2 F] */
  float* xcat;        /* [N, 2 F] */
  float* gEN;         /* [N, F] */
  /* parameter-gradient sweeps: slots [2][dir_stride] (written by TRAIN_NBR / TRAIN_FILTER, read by TRAIN_GPRE) */
  float* slots;
  float* self_rows;      /* [N, Wd] */
  const float* self_sum; /* [Wd] */
  const float* pre;      /* [P + 1, Wd] */
  float* g_pre;          /* [P + 1, Wd] */
} tmdnet_et_unit_args;
int tmdnet_debug_et(void* stream, const tmdnet_et_unit_args* args, int32_t* route_out);

/* ---- First-order parameter gradients (TensorNet, TensorNet2 and Equivariant Transformer handles; energy-only training).
 * Replaces what autograd does in the reference for `loss(E).backward()` over torchmdnet/models/tensornet.py:543-619, 729-814,
 * 384-398 and output_modules.py:108-117: given d loss / d E_m per molecule, one call evaluates the energies (direct evaluation
 * of the radial functions, no tables) and the gradient of sum_m grad_energy[m] E_m with respect to every weight, into one flat
 * device buffer whose layout tmdnet_param_grad_entry enumerates (name, offset and element count; offsets are 64-float
 * aligned).  Entry names are the engine's: "Wdp"/"bdp" = distance_proj1..3 stacked, "Utab"/"Vtab" = the per-species tables
 * U[z] = emb(z) Wa^T + b, V[z] = emb(z) Wb^T of emb2([emb(z_i), emb(z_j)]) (chain to emb / emb2 on the caller's side),
 * "Ue{k}", "L1", "bL1", "L2", "bL2", "ln0_w", "ln0_b" = tensor_embedding linears_tensor / linears_scalar / init_norm,
 * "l{l}.M{k}", "l{l}.b{k}" = layers.l.linears_scalar.k, "l{l}.Va{k}" / "l{l}.Vb{k}" = layers.l.linears_tensor.k / .(3+k),
 * "lnr_w", "lnr_b" = out_norm, "Lin", "bLin" = linear, "O1", "bO1", "O2", "bO2" = output_network.layers.0 / .2.
 * TensorNet2 handles add "l{l}.M0b" / "l{l}.M0c" (charge blocks of linears_scalar.0) and "cp{h}.ln_w", "cp{h}.W1" ... (ChargePredict).
 * Equivariant Transformer handles enumerate their own entries ("emb", "embN", "Wn", "bn", "Wc", "bc", "l{l}.ln_w", "l{l}.Wqkv" =
 * q | k | v rows as packed by the engine, "l{l}.Wvp", "l{l}.Wo", "l{l}.Wdkv" = dk_proj | dv_proj, "lno_w", "W1u", "Wm1", "Wm2", "W21",
 * "Wn1", "Wn2", ...; torchmdnet_amd/models/model.py::_et_grads maps them back) and take the one-call form only.
 * Needs a graph built with the exact pair count (tmdnet_build_graph, no cell list); deterministic; no position gradient.
 * Two-call form for autograd: grad_energy == NULL runs the forward half only (energies out, activations kept in ws / train_ws),
 * a later call with energy == NULL and the same other arguments runs the reverse half on those workspaces. */
int tmdnet_param_grad_count(tmdnet_model* m);
const char* tmdnet_param_grad_entry(tmdnet_model* m, int idx, int64_t* offset, int64_t* numel);
int tmdnet_train_workspace_bytes(tmdnet_model* m, int64_t n_atoms, int64_t n_mol, int64_t n_pairs, size_t* fwd_bytes,
                                 size_t* train_bytes, int64_t* grad_floats);
int tmdnet_energy_param_grads(tmdnet_model* m, void* stream, void* graph_ws, void* ws, size_t ws_bytes, void* train_ws,
                              size_t train_bytes, int64_t n_atoms, int64_t n_mol, int64_t n_pairs, const int64_t* z,
                              const int64_t* batch, const float* q, const float* grad_energy, float* energy, float* grads);

/* Second-order pass of force-matching training (TensorNet + Scalar, Equivariant Transformer): the gradient, with respect to every weight, of
 *     s(theta) = v . d(sum_m E_m)/d pos = - v . F          v [n_atoms, 3] = d loss / d F  (device, caller's atom order)
 * so that d loss / d theta through the forces is  - grads.  Replaces the reference's second autograd pass over its own graph
 * (torchmdnet/models/model.py:618-628, create_graph = self.training) and the *_bwd_bwd kernels behind it
 * (torchmdnet/extensions/warp_ops/tensornet_mp.py:538-548 and siblings).  Analytic: the forward-mode tangent, along v, of the
 * forward + reverse program (no difference quotient); one self-contained pass that evaluates the radial functions directly and
 * keeps its own activations in `ws` (tmdnet_force_param_workspace_bytes: about 2 KB per atom-channel plus 0.4 KB per
 * pair-channel, 14 GiB for 256 molecules of 64 atoms at 128 channels - nothing is aliased).  `grads` has the layout of tmdnet_energy_param_grads (tmdnet_param_grad_entry; d s / d bO2 = 0).  Needs a graph
 * built with the exact pair count and without the cell list; `z` may be NULL when tmdnet_build_graph saw it; deterministic.
 * `hv` (device, [n_atoms, 3], or NULL): d s / d pos = H v, the Hessian of the summed energy applied to v - the position gradient
 * of a loss that depends on the forces is  - H (d loss / d F)  (the reference gets it from the same second autograd pass). */
int tmdnet_force_param_workspace_bytes(tmdnet_model* m, int64_t n_atoms, int64_t n_mol, int64_t n_pairs, size_t* bytes);
int tmdnet_force_param_grads(tmdnet_model* m, void* stream, void* graph_ws, void* ws, size_t ws_bytes, int64_t n_atoms,
                             int64_t n_mol, int64_t n_pairs, const int64_t* z, const int64_t* batch, const float* q, const float* v,
                             float* grads, float* hv);
/* The whole gradient of a loss(E, F) in ONE pass: tmdnet_force_param_grads with an energy seed.  ge [n_mol] = d loss / d E (device;
 * NULL = tmdnet_force_param_grads): grads = d S / d theta and hv = d S / d pos of
 *     S = v . d(sum_m E_m)/d pos - sum_m ge_m E_m ,
 * so d loss / d theta = - grads and d loss / d pos = - hv, without the separate tmdnet_energy_param_grads pass (the reference gets
 * both terms from one backward over its autograd graph, torchmdnet/models/model.py:618-628).  How: the tangent adjoint minus the
 * adjoint of sum_m ge_m E_m obeys the tangent adjoint's own recursion, so only its seed at the head differs.  Terms outside the
 * engine's parameter set (an Atomref prior's table: index_add of ge[molecule] over z) stay with the caller. */
int tmdnet_loss_param_grads(tmdnet_model* m, void* stream, void* graph_ws, void* ws, size_t ws_bytes, int64_t n_atoms, int64_t n_mol,
                            int64_t n_pairs, const int64_t* z, const int64_t* batch, const float* q, const float* v, const float* ge,
                            float* grads, float* hv);
/* Developer / test hook: copies one intermediate of the LAST tmdnet_force_param_grads call on this handle (same thread, workspace
 * untouched since) into `out` (device); names are the buffer names of csrc/tn_hvp_api.hip ("u0_t", "l0.Mi_t", "g_Pn", ...).
 * out == NULL: returns the element count instead of a status. */
int tmdnet_hvp_debug_tensor(tmdnet_model* m, void* stream, const char* name, float* out, int64_t numel);

/* ---- Device-resident molecular dynamics (csrc/tn_md.hip; additive exports, the ABI revision stays 10) ------------------------
 * The integrator launches that sit between two tmdnet_energy_forces calls of a captured step, so that K full MD steps replay as
 * one HIP graph without host work in between (the reference has no counterpart: its MD loops live in the caller's Python).
 * Scheme, per atom i, with hk_i = dt force_scale / (2 m_i):
 *     v <- v + hk_i F    x <- x + dt v    F = F(x)    v <- v + hk_i F    [ v <- c1 v + c2 sigma_i xi ]
 * Units: whatever the caller's are, as long as force_scale turns [F] / [m] into [x] / [dt]^2 - with eV, Angstrom, amu and fs,
 * force_scale = 9.648533e-3 (1 eV / (Angstrom amu) = 9.648533e-3 Angstrom / fs^2).  `pos` is never wrapped: the engine takes
 * unwrapped positions.  sigma_i = sqrt(kT force_scale / m_i) is the thermal velocity, c1 = exp(-gamma dt), c2 = sqrt(1 - c1^2).
 * An atom with m = inf (hk = sigma = 0) and zero velocity is frozen: its position and velocity keep their bits, and it
 * adds nothing to the kinetic energy.
 * Rounding contract: every product and every sum above is a single round-to-nearest fp32 operation in the order written (hk F,
 * then + v; dt v, then + x; c1 v, c2 sigma, that times xi, then the sum), never contracted into an FMA and never reassociated; a
 * launch that closes one step and opens the next performs the two kicks as two additions.  Without a thermostat a trajectory is
 * therefore bit-identical to any fp32 mirror that evaluates the same operations one by one on the same forces.
 * Noise: Philox4x32-10, key = `seed` (low word first), counter = (step low, step high, atom index in the CALLER's order, 0)
 * with `step` the number of steps completed before this one; words 0 / 1 give (xi_x, xi_y) by Box-Muller, words 2 / 3 give xi_z
 * (cosine branch), from u = ((word >> 8) + 0.5) 2^-24 and the accurate logf / cosf / sinf.  It depends on (seed, step, atom) only.
 * All pointers are caller-owned device memory unless stated; nothing allocates, and only tmdnet_md_status synchronises. */
#define TMDNET_MD_OPEN 0   /* B, A of the first step of a replay (reads `forces` of the state the loop starts from) */
#define TMDNET_MD_MIDDLE 1 /* after an evaluation: B [, O], kinetic energy of that step, then B, A of the next, in one launch */
#define TMDNET_MD_CLOSE 2  /* after the last evaluation: B [, O], kinetic energy */
/* Bytes of the MD state `md_ws` for n_atoms atoms in n_mol molecules: a 256-byte header (64-bit step counter, sticky status),
 * the positions and velocities of the last completed step (24 bytes per atom), 4 bytes per atom of kinetic-energy terms and the
 * slice sums of molecules above 1 024 atoms. */
int tmdnet_md_workspace_bytes(int64_t n_atoms, int64_t n_mol, size_t* bytes);
/* Enqueues: step counter = step0, status = 0.  Required once before the first tmdnet_md_advance on a workspace. */
int tmdnet_md_reset(void* stream, void* md_ws, uint64_t step0);
/* Enqueues one integrator launch (TMDNET_MD_MIDDLE / _CLOSE: plus the per-molecule reduction of the kinetic energy, one launch,
 * two when a molecule has more than 1 024 atoms on average).  K steps are OPEN, then K times { evaluation at `pos`; MIDDLE, or CLOSE
 * after the last }.
 *   m, graph_ws   the handle and graph workspace of the evaluation before this launch: its overflow flag is read, and the atom
 *                 ranges of the molecules are taken from it.  graph_ws == NULL (m may then be NULL): no overflow test, the
 *                 kinetic energy is summed over `batch` (NULL: one molecule).
 *   pos, vel      [n_atoms, 3], updated in place.
 *   forces        [n_atoms, 3], read only: any buffer, the evaluation's output or the caller's own.
 *   energy        [n_mol] or NULL: copied to epot_log_row (the next evaluation overwrites it).
 *   hk, mass, sigma   [n_atoms]; sigma == NULL: no thermostat (c1, c2, seed unused); mass is read by MIDDLE / CLOSE only.
 *   batch         [n_atoms] int64 molecule index in the caller's order, or NULL.
 *   forces_keep   [n_atoms, 3] or NULL: MIDDLE / CLOSE copy `forces` here, so that a buffer the caller owns always holds the
 *                 forces at the last completed step (the `forces` of the next replay's OPEN).
 *   epot_log_row, ekin_log_row   [n_mol] each, or NULL: energies of the step just completed; ekin = sum of 0.5 m v^2 after the
 *                 closing kick and the O step, in the unit of m v^2 (divide by force_scale for the unit of the energies), summed
 *                 in a fixed order without floating-point atomics: bit-identical repeats.
 * Overflow: when the evaluation before a MIDDLE / CLOSE launch overflowed (static shapes: its forces are stale), pos and vel go
 * back to the last completed step and the status word is set; from then on every launch leaves pos, vel, forces_keep, the log
 * rows and the step counter alone, until tmdnet_md_reset. */
int tmdnet_md_advance(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, int64_t n_atoms, int64_t n_mol, int32_t phase,
                      float* pos, float* vel, const float* forces, const float* energy, const float* hk, const float* mass,
                      const float* sigma, float dt, float c1, float c2, uint64_t seed, const int64_t* batch, float* forces_keep,
                      float* epot_log_row, float* ekin_log_row);
/* host[0] = steps completed (the device counter), host[1] = status (1: an evaluation overflowed; the state is that of step
 * host[0].  2: a barostat move was unusable, see tmdnet_md_barostat and tmdnet_md_barostat_cell; step host[0] is complete but for
 * that move.  3: a constraint
 * cluster did not converge, see tmdnet_md_advance_constrained.  4: a walker's collective variable, its gradient or its bias was not
 * finite, see tmdnet_md_bias; the state is half a step ahead of step host[0].  5: a move of a global thermostat was unusable, see
 * tmdnet_md_thermostat; step host[0] is complete but for that move).  Synchronises the stream.  Returns TMDNET_ERR_OVERFLOW for
 * status 1 and TMDNET_ERR_STATE for status 2, 3 and 4, and for status 5 likewise. */
int tmdnet_md_status(void* stream, void* md_ws, uint64_t host[2]);

/* ---- Barostat of the device-resident MD loop (csrc/tn_md.hip; additive exports, the ABI revision stays 10) --------------------
 * Isotropic stochastic cell rescaling (Bernetti and Bussi, J. Chem. Phys. 153, 114107, 2020), one barostat per molecule (replica),
 * first order in the log-volume.  After the closing half of a step (tmdnet_md_advance with TMDNET_MD_CLOSE), per molecule m, in fp64:
 *     V  = |det box_m|                                  K = ekin_row[m] / force_scale
 *     P  = (2 K + W_m[0][0] + W_m[1][1] + W_m[2][2]) / (3 V)         (W of tmdnet_energy_forces_virial: tr W = -3 V dE/dV)
 *     a  = compressibility dt / tau                      d = -a (P0 - P) + sqrt(2 kT a / V) xi
 *     mu = exp(d / 3), nu = exp(-d / 3), both rounded to fp32 once
 * then box_m <- box_m mu (all nine entries: any triclinic box), x <- x mu and v <- v nu for the atoms of m, each ONE rounded fp32
 * product under the rounding contract above.  kT = 0 is weak coupling (no noise).  Units: pressure in E / length^3, compressibility
 * in length^3 / E, kT in E (1 bar = 6.2415091e-7 eV / Angstrom^3).  The forces are NOT evaluated again after the scaling: the next
 * opening kick uses F(x) of before the move (first-order splitting).
 * Noise: xi = xi_x of the Box-Muller map above on one Philox4x32-10 call, key = `seed`, counter = (step low, step high, molecule,
 * 1) with `step` the value the O step of this MD step used; counter word 3 keeps the stream apart from the atoms' (0).
 * Enqueues two launches: one block that computes every molecule's move and, when all are usable, writes the factors, scales the
 * boxes and fills the log rows; then one thread per atom that scales x and v and, with open_next != 0, saves the scaled state and
 * runs B, A of the next step on it (what TMDNET_MD_OPEN does).  A captured step with a barostat is therefore
 *     evaluation with the virial;  tmdnet_md_advance(TMDNET_MD_CLOSE);  tmdnet_md_barostat(open_next = another step follows)
 * after one TMDNET_MD_OPEN at the start of the replay; TMDNET_MD_MIDDLE is not used (the kinetic energy of the closing half has to
 * be reduced before the move).
 *   m, graph_ws   as in tmdnet_md_advance: when the evaluation overflowed, nothing is written (the CLOSE launch before has latched
 *                 status 1, so the box is always that of the last completed step).  graph_ws == NULL (m may be NULL): no such test.
 *   baro_ws       tmdnet_md_barostat_workspace_bytes(n_mol) bytes of scratch: the factors mu | nu of every molecule.
 *   forces, hk, dt   read with open_next only.
 *   batch         [n_atoms] int64 or NULL (one molecule), as in tmdnet_md_advance.
 *   box, box_mode    2: [n_mol, 3, 3], one box per molecule; 1: one [3, 3] box, n_mol == 1 only.  Scaled in place.
 *   virial        [n_mol, 3, 3] of the evaluation of this step;  ekin_row   [n_mol], the ekin_log_row of the CLOSE launch.
 *   volume_log_row, pressure_log_row, scale_log_row   [n_mol] each or NULL: V before the move, P, and mu as fp32.
 * A move is unusable when V = 0 or anything on the way to mu, nu is not finite (a NaN in the virial): the status word becomes 2,
 * box, pos, vel and the log rows keep their bits, and every later launch returns at once until tmdnet_md_reset.
 * TMDNET_ERR_INVALID: box_mode 0, box_mode 1 with n_mol > 1, tau <= 0, compressibility <= 0, kT < 0, force_scale <= 0, or a NULL
 * box / virial / ekin_row / workspace. */
int tmdnet_md_barostat_workspace_bytes(int64_t n_mol, size_t* bytes);
int tmdnet_md_barostat(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* baro_ws, int64_t n_atoms, int64_t n_mol,
                       int32_t open_next, float* pos, float* vel, const float* forces, const float* hk, float dt, const int64_t* batch,
                       float* box, int32_t box_mode, const float* virial, const float* ekin_row, double pressure, double kT,
                       double compressibility, double tau, double force_scale, uint64_t seed, float* volume_log_row,
                       float* pressure_log_row, float* scale_log_row);

/* ---- Anisotropic cell rescaling of the device-resident MD loop (csrc/tn_md_cell.hip; additive exports, the ABI revision stays 10)
 * The barostat above with a 3 x 3 matrix in the exponent, so that the SHAPE of the cell fluctuates: the anisotropic stochastic cell
 * rescaling of Bernetti and Bussi (J. Chem. Phys. 153, 114107, 2020), one barostat per molecule, first order.  After the closing
 * half of a step (tmdnet_md_advance with TMDNET_MD_CLOSE), per molecule m, in fp64, row vectors, h = box_m:
 *     V   = |det h|                                  Kt = sum over the atoms of m of 0.5 mass v_a v_b / force_scale      (3 x 3)
 *     P   = (2 Kt + W_m) / V                         (W of tmdnet_energy_forces_virial as returned, not symmetrised)
 *     a   = compressibility dt / tau                 D_f = -(a / 3) (P0 I - P) + sqrt(2 kT a / (3 V)) Xi     (Xi: 9 standard normals)
 *     D   = Pi(D_f)       mu = exp(D)       nu = exp(-D^T)                                                   (matrix exponentials)
 * Pi projects onto the coupling's subspace (Frobenius-orthogonally):
 *   TMDNET_CELL_ANISOTROPIC      the identity: all nine entries
 *   TMDNET_CELL_DIAGONAL         the three diagonal entries; the off-diagonal ones are 0
 *   TMDNET_CELL_SEMI_ISOTROPIC   diagonal, and the two entries other than `axis` are replaced by their mean
 * Written in the exponent the Ito term of exp cancels the paper's + kT / V, so the drift is -(a / 3) (P0 - P) alone; tr D is
 * distributed as the d of tmdnet_md_barostat in every mode.  kT = 0 is anisotropic weak coupling.  The matrix exponential scales D
 * by 2^-s to a max-row-sum norm <= 2^-4, sums the Taylor series to degree 8 and squares s times; nu is the same routine on -D^T.
 * Lower-triangular box (ANISOTROPIC only): h mu = L Q by Gram-Schmidt on its rows, top down, q2 = q0 x q1 (L lower triangular with a
 * positive diagonal), and the whole system is rotated by Q^T:  box <- L,  x <- x (mu Q^T),  v <- v (nu Q^T),  F <- F Q^T  for the
 * forces of the last evaluation (the opening kick of the next step and forces_keep; the energy is invariant).  In the two diagonal
 * modes Q = I: box <- h mu, the matrices are diagonal (scalar exponentials) and the forces are not touched.  The forces are NOT
 * evaluated again after the move, as for tmdnet_md_barostat.
 * Rounding: Mx = mu Q^T, Mv = nu Q^T, Mf = Q^T and the new box are rounded to fp32 ONCE; every per-atom component is then
 * ((x0 M0b) + (x1 M1b)) + (x2 M2b), each product and each sum one rounded fp32 operation in that order under the contract above
 * (ONE product x_b M_bb in the diagonal modes).
 * Noise: row r of Xi is the Box-Muller triple of one Philox4x32-10 call, key = `seed`, counter = (step low, step high, molecule,
 * 4 + r) with `step` the value the O step of this MD step used.  Counter word 3: 0 the atoms, 1 tmdnet_md_barostat, 2
 * tmdnet_md_exchange, 3 + 256 draw tmdnet_md_thermostat, 4 / 5 / 6 the three rows of Xi.
 * Enqueues three launches (four when a molecule averages more than 1 024 atoms): the kinetic tensor per molecule, read from vel and
 * mass and summed in fp64 in a fixed order without floating-point atomics (bit-identical repeats); one block that computes every
 * molecule's move and, when all are usable, writes the matrices, the boxes and the log rows; one thread per atom that applies the
 * matrices and, with open_next != 0, saves the scaled state and runs B, A of the next step on it.  A captured step is therefore
 *     evaluation with the virial;  tmdnet_md_advance(TMDNET_MD_CLOSE);  tmdnet_md_barostat_cell(open_next = another step follows)
 *   m, graph_ws, batch, box, box_mode, virial, hk, dt   as in tmdnet_md_barostat.
 *   cell_ws       tmdnet_md_barostat_cell_workspace_bytes(n_atoms, n_mol) bytes of scratch.  After aligning the pointer up to 256
 *                 bytes it starts with the matrices [n_mol, 27] fp32: Mx | Mv | Mf of every molecule, row-major 3 x 3 each.
 *   mass          [n_atoms]: an atom of infinite mass contributes nothing to Kt.
 *   forces        the forces of this step's evaluation; read with open_next only.
 *   forces_keep   [n_atoms, 3] or NULL, in / out (ANISOTROPIC only): with open_next the rotated `forces` are stored here; without,
 *                 it is rotated in place.  The diagonal modes leave it alone.
 *   volume_log_row [n_mol], pressure_log_row [n_mol, 9], scale_log_row [n_mol, 9], each or NULL: V before the move, P and Mx as fp32.
 * A move is unusable when V = 0, anything on the way to the matrices and the new box is not finite (a NaN in the virial), or
 * det (h mu) <= 0 (a left-handed box): the status word becomes 2, box, pos, vel, forces_keep and the log rows keep their bits, and
 * every later launch returns at once until tmdnet_md_reset.
 * TMDNET_ERR_INVALID: what tmdnet_md_barostat refuses, a NULL mass, a coupling other than the three above, or an axis outside 0..2. */
#define TMDNET_CELL_ANISOTROPIC 0
#define TMDNET_CELL_DIAGONAL 1
#define TMDNET_CELL_SEMI_ISOTROPIC 2
int tmdnet_md_barostat_cell_workspace_bytes(int64_t n_atoms, int64_t n_mol, size_t* bytes);
int tmdnet_md_barostat_cell(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* cell_ws, int64_t n_atoms, int64_t n_mol,
                            int32_t open_next, float* pos, float* vel, const float* forces, const float* hk, const float* mass, float dt,
                            const int64_t* batch, float* box, int32_t box_mode, const float* virial, double pressure, double kT,
                            double compressibility, double tau, double force_scale, uint64_t seed, int32_t coupling, int32_t axis,
                            float* forces_keep, float* volume_log_row, float* pressure_log_row, float* scale_log_row);

/* ---- Temperature replica exchange of the device-resident MD loop (csrc/tn_remd.hip; additive exports, the ABI revision stays 10) -
 * Parallel tempering inside the captured graph.  n_mol = G * ladder replicas of ONE system (n = n_atoms / n_mol atoms each, replica
 * b owns atoms b n .. b n + n - 1 in the caller's order): G independent ladders of R = ladder temperature slots, replica
 * b = g R + r starts in slot r.  Replicas swap TEMPERATURES, not coordinates, so nothing of size n_atoms moves: `slot[b]` (int32)
 * is the slot replica b holds and `holder[g][s]` (int32, 0..R-1 within the ladder) its inverse, both permutations at all times.
 * The ladder need not be monotonic; neighbours are neighbours in the given order.
 * When: a captured step that ends with an attempt is
 *     evaluation;  tmdnet_md_advance(TMDNET_MD_CLOSE);  tmdnet_md_exchange;  tmdnet_md_advance(TMDNET_MD_OPEN, forces = forces_keep)
 * in place of TMDNET_MD_MIDDLE - by the rounding contract CLOSE then OPEN is bit-identical to MIDDLE, so the steps themselves do not
 * change.  The CLOSE reduction has advanced the step counter, which therefore reads n, the number of completed steps.
 * Which pairs: attempt a = n / exchange_every (integer division) tries the slot pairs (s, s + 1) for s = (a & 1), (a & 1) + 2, ...
 * while s + 1 < R.
 * Decision, per pair, with i = holder[g][s], j = holder[g][s + 1] and E = epot_row, in fp64 in the order written:
 *     D = (beta[s] - beta[s + 1]) * ((double)E_i - (double)E_j)          accept iff D >= 0 || (double)u < exp(D)
 * A NaN on the way makes both comparisons false: a rejection, never a status.
 * Noise: u = ((word 0 >> 8) + 0.5) 2^-24 of one Philox4x32-10 call, key = `seed`, counter = (n low, n high, g (R - 1) + s, 2);
 * counter word 3 keeps the stream apart from the atoms' (0) and the barostat's (1).
 * On acceptance: slot[i] <-> slot[j], holder updated; every velocity component of the atoms of i is multiplied by scale_up[s] =
 * fp32(sqrt(kT[s + 1] / kT[s])) and of j by scale_down[s] = fp32(sqrt(kT[s] / kT[s + 1])) (the caller computes both in fp64 and
 * rounds once; each scaling is ONE rounded fp32 product), and sigma[b n + a] <- sigma_table[new slot][a], the caller's table of
 * fp32(sqrt(kT[s] force_scale / m_a)).  An atom of infinite mass has sigma_table = 0 and its zero velocity keeps its bits.
 * Frozen state: when the status word is set, or the evaluation of this step overflowed (graph_ws), the exchange writes nothing - no
 * slot, no velocity, no sigma, no log row and no counter.
 * Enqueues two launches: one lane per slot of every ladder (the lane of a tried pair's lower slot decides and keeps the books),
 * then one thread per atom (velocities and sigma).  No atomics: the result is a function of (seed, n, energies).
 *   m, graph_ws   as in tmdnet_md_barostat.  graph_ws == NULL (m may be NULL): no overflow test.
 *   ex_ws         tmdnet_md_exchange_workspace_bytes(n_mol, ladder) bytes of scratch: one accept flag per pair.
 *   vel [n_atoms, 3], sigma [n_atoms]   updated in place;   epot_row [n_mol]   the epot_log_row of the CLOSE launch.
 *   beta [ladder] double = 1 / kT;  sigma_table [ladder, n];  scale_up, scale_down [ladder - 1].
 *   slot [n_mol], holder [G, ladder]   int32, updated in place.
 *   slot_log_row [n_mol] int32 or NULL: slot of every replica after the attempt.   accept_log_row [G, ladder - 1] uint8 or NULL:
 *                 1 for an accepted pair, 0 for a rejected one and for the pairs not tried in this parity.
 *   counters      [2, G, ladder - 1] int64 or NULL: attempts, then accepts, cumulative (plain adds by the pair's one lane).
 * TMDNET_ERR_INVALID: ladder < 2, n_mol % ladder != 0, n_atoms % n_mol != 0, exchange_every < 1, or a NULL md_ws / ex_ws / vel /
 * sigma / epot_row / beta / sigma_table / scale_up / scale_down / slot / holder. */
int tmdnet_md_exchange_workspace_bytes(int64_t n_mol, int32_t ladder, size_t* bytes);
int tmdnet_md_exchange(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* ex_ws, int64_t n_atoms, int64_t n_mol,
                       int32_t ladder, int64_t exchange_every, float* vel, float* sigma, const float* epot_row, const double* beta,
                       const float* sigma_table, const float* scale_up, const float* scale_down, uint64_t seed, int32_t* slot,
                       int32_t* holder, int32_t* slot_log_row, uint8_t* accept_log_row, int64_t* counters);

/* ---- Global thermostats of the device-resident MD loop (csrc/tn_md_thermo.hip; additive exports, the ABI revision stays 10) -----
 * One thermostat per molecule (replica) that acts on the molecule's kinetic energy through ONE scale factor alpha per step and so
 * leaves the relative motion of the atoms alone.  After the closing half of a step (tmdnet_md_advance with TMDNET_MD_CLOSE and no
 * Langevin thermostat), per molecule m, in fp64 in the order written in csrc/tn_md_thermo_math.h, with K = ekin_row[m] / force_scale
 * and N = ndof[m]:
 *   TMDNET_THERMOSTAT_CSVR   stochastic velocity rescaling (Bussi, Donadio, Parrinello, J. Chem. Phys. 126, 014101, 2007):
 *       c = exp(-dt / tau), r = (N kT / 2) / (N K), alpha^2 = (sqrt(c) + R1 sqrt(r (1 - c)))^2 + r (1 - c) S
 *     R1 a standard normal and S chi-square with N - 1 degrees of freedom (2 Gamma((N - 1) / 2) for N - 1 even, 2 Gamma((N - 2) / 2)
 *     + R2^2 for N - 1 odd; the gamma deviate is Marsaglia and Tsang's, at most 64 attempts).  reservoir -= (alpha^2 - 1) K.
 *   TMDNET_THERMOSTAT_NHC    a Nose-Hoover chain of `chain` thermostats (Martyna, Klein, Tuckerman, J. Chem. Phys. 97, 2635, 1992)
 *     with Q_1 = N kT tau^2 and Q_j = kT tau^2, propagated by `substeps` applications of the chain routine of Martyna, Tuckerman,
 *     Tobias and Klein (Mol. Phys. 87, 1117, 1996) with h = dt / substeps; alpha is the accumulated scale.
 *     reservoir = sum_j Q_j v_j^2 / 2 + N kT xi_1 + kT sum_{j >= 2} xi_j.
 * alpha is rounded to fp32 once; then v <- v alpha for the atoms of m, ONE rounded fp32 product per component under the rounding
 * contract above.  An atom of infinite mass (hk = 0) carries no kinetic energy and keeps its velocity bit for bit.  A molecule with
 * ndof <= 0 or K = 0 is not scaled: alpha = 1, no random number, state untouched.  kT in the unit of E, tau in the unit of dt.
 * Noise: Philox4x32-10, key = `seed`, counter = (step low, step high, molecule, 3 + 256 draw) with `step` the value the O step of
 * this MD step would use; draw 0 gives R1 = xi_x and R2 = xi_y of the Box-Muller map above, draw j >= 1 is attempt j of the gamma
 * deviate (x = xi_x, u from word 2).  Counter word 3 keeps the stream apart from the atoms' (0), the barostat's (1) and the
 * exchange's (2).
 * Enqueues two launches: one block that computes every molecule's move and, when all are usable, writes the factors, the reservoir,
 * the chain and the log rows; then one thread per atom that scales v and, with open_next != 0, saves the scaled state and runs B, A
 * of the next step on it (what TMDNET_MD_OPEN does).  A captured step with a global thermostat is therefore
 *     evaluation;  tmdnet_md_advance(TMDNET_MD_CLOSE);  tmdnet_md_thermostat(open_next = another step follows)
 * after one TMDNET_MD_OPEN at the start of the replay.  With constraints open_next = 0 and tmdnet_md_advance_constrained(OPEN)
 * follows: a uniform scaling of a molecule's velocities keeps them on the constraints.
 *   m, graph_ws   as in tmdnet_md_barostat.  graph_ws == NULL (m may be NULL): no overflow test.
 *   thermo_ws     tmdnet_md_thermostat_workspace_bytes(n_mol, chain) bytes, zeroed by the caller before the first move and to
 *                 reset the thermostat; after aligning the pointer up to 256 bytes: alpha fp32 [n_mol], then (each part rounded up
 *                 to 256 bytes) the reservoir fp64 [n_mol] and the chain fp64 [n_mol, 2, chain] = (xi | v_xi).
 *   forces, dt    read with open_next only;  hk [n_atoms] always (it tells the atoms of infinite mass);  pos   with open_next only.
 *   batch         [n_atoms] int64 or NULL (one molecule).   ekin_row   [n_mol], the ekin_log_row of the CLOSE launch.
 *   ndof          [n_mol] int32: the degrees of freedom of every molecule.
 *   chain, substeps   NHC only (CSVR: ignored, its workspace is sized with chain = 0).
 *   scale_log_row [n_mol] fp32 or NULL: alpha.   reservoir_log_row [n_mol] fp64 or NULL: the reservoir after the move, unit of E.
 * A move is unusable when K, alpha or a chain value is not finite, alpha <= 0, or the gamma deviate used up its attempts: the status
 * word becomes 5, no factor, reservoir, chain value or log row is written for ANY molecule, vel keeps its bits, and every later
 * launch returns at once until tmdnet_md_reset.
 * TMDNET_ERR_INVALID: an unknown kind, tau <= 0, kT <= 0, force_scale <= 0, NHC with chain outside 1..8 or substeps < 1, or a NULL
 * md_ws / thermo_ws / vel / hk / ekin_row / ndof (with open_next: pos / forces). */
#define TMDNET_THERMOSTAT_CSVR 0
#define TMDNET_THERMOSTAT_NHC 1
int tmdnet_md_thermostat_workspace_bytes(int64_t n_mol, int32_t chain, size_t* bytes);
int tmdnet_md_thermostat(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* thermo_ws, int64_t n_atoms, int64_t n_mol,
                         int32_t kind, int32_t open_next, float* pos, float* vel, const float* forces, const float* hk, float dt,
                         const int64_t* batch, const float* ekin_row, const int32_t* ndof, double kT, double tau, int32_t chain,
                         int32_t substeps, double force_scale, uint64_t seed, float* scale_log_row, double* reservoir_log_row);

/* ---- Collective-variable restraints and metadynamics of the device-resident MD loop (csrc/tn_bias.hip; additive exports, the ABI
 * revision stays 10) ------------------------------------------------------------------------------------------------------------
 * Enhanced sampling inside the captured graph: ONE launch between the evaluation of a step and the integrator launch that closes
 * it adds a bias force to the evaluation's force buffer in place, so a captured step is
 *     evaluation;  tmdnet_md_bias(forces = the evaluation's output);  tmdnet_md_advance(TMDNET_MD_MIDDLE or _CLOSE, the same forces)
 * The n_mol molecules are walkers.  Every walker has the same n_cv <= 8 collective variables (CVs), on atoms given relative to the
 * first atom of its molecule (mol_start); positions are the unwrapped ones, no minimum image is applied.  In fp64 on the fp32
 * positions (csrc/tn_bias_math.h):
 *     kind 0  distance(i, j)       |x_i - x_j|
 *     kind 1  angle(i, j, k)       atan2(|r1 x r2|, r1.r2) at j, radians
 *     kind 2  torsion(i, j, k, l)  in (-pi, pi], IUPAC sign, by atan2; gradients in the Blondel-Karplus form (no 1 / sin)
 * diff(a, b) = a - b, for a torsion wrapped into (-pi, pi].
 * Restraints, one per CV (restraint_kind 0: none): V = 0.5 kappa D^2 with D = diff(s, center); kind 1 harmonic, 2 upper (D > 0
 * only), 3 lower (D < 0 only); kappa and center are [n_mol, n_cv] doubles: umbrella windows are one batch.
 * Metadynamics on n_metad_cv = 1 or 2 of the CVs (0: none): consecutive walkers form groups of walkers_per_group = W that share
 * one list of `capacity` = H hills, V(s) = sum_h w_h exp(-sum_d diff(s_d, c_hd)^2 / (2 sigma_d^2)), no truncation and no grid.
 * Which hills exist: n is the step counter of md_ws, which only the closing launch advances; step0 and hill_base are what
 * tmdnet_md_bias_reset wrote.  A launch reads the slots below hill_base + ((n - step0) / pace) W (at most H).  With deposit != 0
 * and (n + 1 - step0) % pace == 0, walker w of a group writes slot hill_base + ((n + 1 - step0) / pace - 1) W + w: its centre is
 * the walker's s, its height h0 exp(-V(s) / (kT (bias_factor - 1))) with the V(s) this launch computed (well-tempered), or h0 when
 * bias_factor == 0 (plain).  A slot >= H is not written.  No launch reads a slot it writes, and there is no counter to race on.
 * deposit == 0 only evaluates (the forces of a start geometry).
 * Force: per distinct atom of a walker the fp64 sum, in CV order and then slot order, of -dV/ds_cv * ds_cv/dx over the entries
 * that name it, rounded to fp32 ONCE and added to forces[atom] with ONE rounded fp32 addition under the rounding contract above.
 * Atoms in no CV keep their bits.  The reduction over the hills has a fixed order (a thread strides by 256, lanes add by the wave
 * xor tree, waves in turn), without floating-point atomics: repeats are bit-identical.
 * Frozen state: when the status word is set, or the evaluation of this step overflowed (graph_ws), nothing is written.  A walker
 * whose CV, gradient, bias or force is not finite (coincident atoms, a collinear angle or torsion, a NaN position, an atom index
 * outside the batch) leaves its forces alone, deposits nothing, writes no log row and stores status 4: the closing launch that
 * follows then returns at once, the state stays finite and half a step ahead of the last completed step, until tmdnet_md_reset.
 * Enqueues one launch, one block of 256 threads per walker.
 *   bias_ws       tmdnet_md_bias_workspace_bytes(...) bytes, aligned up to 256 by the callee: a 256-byte header (uint64 step0,
 *                 uint64 hill_base), then per group (n_metad_cv + 1) arrays of H doubles: centre 0 [, centre 1], height.
 *   pos [n_atoms, 3] read;  forces [n_atoms, 3] updated in place.
 *   cv_kind [n_cv], cv_atoms [n_cv, 4] (unused slots are not read), mol_start [n_mol]   int32.
 *   n_distinct, atom_rel [n_distinct], entry_offsets [n_distinct + 1], entries [32]   int32: the distinct atoms of a walker's
 *                 CVs (relative), and for each the entries (cv << 2 | slot) that name it, in CV order then slot order.
 *   sigma0, sigma1, height, kT, bias_factor, pace   the metadynamics parameters (sigma1 with n_metad_cv == 2 only).
 *   cv_log_row [n_mol, n_cv], restraint_log_row [n_mol], bias_log_row [n_mol]   double or NULL: s, the restraint energy and V(s).
 *   force_log_row [n_mol, n_distinct, 3]   float or NULL: the fp32 bias force of every distinct atom.
 * TMDNET_ERR_INVALID: n_cv outside 1..8, n_distinct outside 1..32, n_metad_cv outside 0..2 or above n_cv, a metad CV out of range
 * or named twice, sigma <= 0, pace < 1, height < 0, bias_factor neither 0 nor > 1, kT <= 0 with a bias factor, W < 1,
 * n_mol % W != 0, capacity < W, or a NULL workspace, position, force or table pointer. */
int tmdnet_md_bias_workspace_bytes(int64_t n_mol, int32_t n_cv, int32_t n_metad_cv, int32_t walkers_per_group, int64_t capacity,
                                   size_t* bytes);
/* Enqueues: the header of bias_ws = (step0, hill_base).  Required once before the first tmdnet_md_bias on a workspace; the hills
 * themselves are the caller's to fill (a restart) or to leave (slots below hill_base must hold hills). */
int tmdnet_md_bias_reset(void* stream, void* bias_ws, uint64_t step0, uint64_t hill_base);
int tmdnet_md_bias(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* bias_ws, int64_t n_atoms, int64_t n_mol,
                   int32_t deposit, const float* pos, float* forces, int32_t n_cv, const int32_t* cv_kind, const int32_t* cv_atoms,
                   const int32_t* mol_start, int32_t n_distinct, const int32_t* atom_rel, const int32_t* entry_offsets,
                   const int32_t* entries, const int32_t* restraint_kind, const double* kappa, const double* center,
                   int32_t n_metad_cv, int32_t metad_cv0, int32_t metad_cv1, double sigma0, double sigma1, double height, double kT,
                   double bias_factor, int64_t pace, int32_t walkers_per_group, int64_t capacity, double* cv_log_row,
                   double* restraint_log_row, double* bias_log_row, float* force_log_row);

/* ---- Observables of the device-resident MD loop (csrc/tn_observe.hip; additive exports, the ABI revision stays 10) -------------
 * Sample frames, the pair-distance histogram g(r), the mean-square displacement and the velocity autocorrelation, recorded inside
 * the captured graph.  The observer sits where the bias launch sits: a sampled step is
 *     evaluation;  tmdnet_md_observe(...);  tmdnet_md_advance(TMDNET_MD_MIDDLE or _CLOSE, ...)
 * It reads pos, vel and the caller's tables and writes ONLY into obs_ws: the trajectory keeps every bit.  At that point the step
 * counter n of md_ws counts the completed steps, pos is x at the full step s = n + 1 and vel is the leapfrog velocity v(s - 1/2)
 * the opening half stored (after the opening kick and, with constraints, after SHAKE's correction).
 * Sampling: s0 is what tmdnet_md_observe_start wrote.  Step s is a sample when s > s0 and (s - s0) % every == 0; its index is
 * j = (s - s0) / every - 1, computed on the device from the 64-bit counter.  The caller enqueues the entry only at the sampling
 * positions of its graph (replay position k with (k + 1) % every == 0 when every divides the steps of a replay), so other steps cost
 * nothing; a launch at a step that is no sample writes nothing.  There is no sample counter on the device: the number of samples
 * recorded is (n - s0) / every for the n tmdnet_md_status reports.
 * Frames (frame_capacity = F > 0): row j % F of a ring of F position frames (and velocity frames with frame_velocities) gets the
 * bits of pos (vel), in the caller's atom order.
 * Histogram (n_pair_types = P in 1..4, bins <= 1024): per molecule and pair type, counts[m][p][bin] += 1 (uint64) for every pair of
 * atoms i < j of molecule m whose selector masks match type p - one atom matches selector a (bit 2p of atom_mask) and the other
 * selector b (bit 2p + 1), in either orientation, once - and whose squared distance d2, the engine's pair geometry in fp32 with the
 * minimum image of that molecule's box (delta = pos[j] - pos[i], fused shifts z -> y -> x), satisfies d2 < r_max2:
 * bin = min((int)(sqrtf(d2) * inv_dr), bins - 1), sqrtf correctly rounded, the product one rounded fp32 multiplication.  The caller
 * passes r_max2 = r_max^2 and inv_dr = bins / r_max, each formed in fp64 and rounded once.  The minimum image is exact only for r_max
 * up to half the smallest height of the box; the caller checks that.  Molecules are contiguous (mol_start, a sorted batch); the
 * caller's table `tiles` holds one row (m, it, jt), jt >= it, per pair of 256-atom tiles of a molecule, one block each.  All adds are
 * integer atomicAdd on LDS and on global memory: sums do not depend on their order, repeats are bit-identical.
 * MSD (n_msd_groups = G in 1..4, msd_capacity = T): msd[j][m][g] = sum over the atoms of molecule m in group g (bit 8 + g of
 * atom_mask) of |pos_i - origin_i|^2 in fp64 on the fp32 values; origin is the pos tmdnet_md_observe_start copied.  Samples j >= T
 * are not written.  The caller divides by the group sizes.
 * VACF (n_vacf_groups = G in 1..4, lags = L <= 256): vel goes into row j % L of a ring; then for every lag l <= min(j, L - 1),
 * acc[m][g][l] += sum over the atoms of molecule m in group g (bit 16 + g) of v_i(j) . v_i(j - l), in fp64.  The caller divides
 * by (n_samples - l) and the group size.
 * fp64 sums have a fixed order (a thread strides by 256, lanes by the wave xor tree, waves in turn), without floating-point
 * atomics.  Frozen state: when the status word of md_ws is set, or the evaluation of this step overflowed (graph_ws), nothing is
 * written.  Enqueues at most three launches: the per-atom copies, the histogram, and a grid (n_mol, 1 + L) for MSD and VACF.
 *   obs_ws        tmdnet_md_observe_workspace_bytes(...) bytes, aligned up to 256 by the callee; arrays, each on a multiple of 256
 *                 bytes, an array that is off taking none: a 256-byte header (uint64 s0), frames pos [F, N, 3] float, frames vel
 *                 [F, N, 3] float, counts [B, P, bins] uint64, origin [N, 3] float, msd [T, B, G] double, ring [L, N, 3] float,
 *                 acc [B, G, L] double.
 *   batch [n_atoms] int64 (NULL: one molecule), box [3, 3] (box_mode 1) or [n_mol, 3, 3] (box_mode 2) or NULL (box_mode 0).
 *   atom_mask [n_atoms] uint32, mol_start [n_mol + 1] int32 and tiles [n_tiles, 3] int32 (both read with n_pair_types > 0 only).
 * TMDNET_ERR_INVALID: every < 1, no observable, more than 4 pair types or groups, bins outside 1..1024, lags outside 1..256,
 * msd_capacity < 1, r_max2 or inv_dr not positive, a box_mode that does not fit box, or a NULL workspace, position, velocity or
 * table pointer. */
typedef struct {
  int32_t every;            /* S: the sampling interval in steps */
  int32_t frame_capacity;   /* F, 0: no frames */
  int32_t frame_velocities; /* != 0: velocity frames too */
  int32_t n_pair_types;     /* P, 0: no histogram */
  int32_t bins;
  float r_max2;
  float inv_dr;
  int32_t n_msd_groups;     /* 0: no MSD */
  int32_t n_vacf_groups;    /* 0: no VACF */
  int32_t lags;             /* L */
  int64_t msd_capacity;     /* T */
} tmdnet_md_observe_spec;
int tmdnet_md_observe_workspace_bytes(int64_t n_atoms, int64_t n_mol, const tmdnet_md_observe_spec* spec, size_t* bytes);
/* Enqueues: the whole workspace zeroed (histogram, logs, accumulators, rings), s0 into its header and pos into origin.  Required
 * once before the first tmdnet_md_observe on a workspace, and again whenever the loop is given new positions or a new step. */
int tmdnet_md_observe_start(void* stream, void* obs_ws, int64_t n_atoms, int64_t n_mol, const tmdnet_md_observe_spec* spec, uint64_t s0,
                            const float* pos);
int tmdnet_md_observe(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* obs_ws, int64_t n_atoms, int64_t n_mol,
                      const tmdnet_md_observe_spec* spec, const float* pos, const float* vel, const int64_t* batch, const float* box,
                      int32_t box_mode, const uint32_t* atom_mask, const int32_t* mol_start, const int32_t* tiles, int64_t n_tiles);

/* ---- Distance constraints of the device-resident MD loop (csrc/tn_md_cons.hip; additive exports, the ABI revision stays 10) ------
 * Holonomic constraints |x_i - x_j| = d_c by RATTLE (Andersen, J. Comput. Phys. 52, 24, 1983) in the splitting above:
 *     B  v <- v + hk F
 *     A  x <- x + dt v
 *     S  SHAKE: x <- x + Dx so that every constraint holds, v <- v + Dx / dt
 *        F = F(x)
 *     B  v <- v + hk F    [ O  v <- c1 v + c2 sigma xi ]
 *     R  RATTLE: v <- v + Dv so that (x_i - x_j).(v_i - v_j) = 0 for every constraint; kinetic energy of the projected v
 * The caller groups the constraints into clusters, the connected components of the constraint graph: at most 8 atoms and 12
 * constraints each.  Atoms in no constraint are packed, up to 8 at a time, into clusters without constraints, so that every atom is in
 * exactly one cluster and goes through the same launch; such an atom gets bit for bit what tmdnet_md_advance gives it (x, v,
 * kinetic term, noise by the caller's atom index).  One group of 8 lanes does a cluster's whole step, so the phases mean what they
 * mean for tmdnet_md_advance and K steps stay K + 1 integrator launches: OPEN = B A S, MIDDLE = B [O] R + kinetic terms, then
 * B A S of the next step, CLOSE = B [O] R + kinetic terms.  TMDNET_MD_PROJECT = R alone at the current positions, no kick and no
 * kinetic energy: once before the first step (and after new velocities), so that velocities drawn from a Maxwell-Boltzmann
 * distribution start consistent with the constraints.
 * The iterations run in fp64 on the cluster's fp32 coordinates, one constraint after the other in table order (Gauss-Seidel), with
 * w = 1 / m from the fp32 masses (1 / inf = 0: that end does not move) and s_c = x_keep_i - x_keep_j, the saved positions of the
 * step's start, as the direction of the SHAKE moves:
 *     S: g = (d^2 - r.r) / (2 (w_a + w_b) s.r),  x_a += g w_a s,  x_b -= g w_b s      until every |r.r - d^2| <= 2 tol d^2
 *     R: k = -r.(v_a - v_b) / ((w_a + w_b) r.r),  v_a += k w_a r,  v_b -= k w_b r     until every |r.(v_a - v_b)| dt <= tol d^2
 * An iteration has converged when one whole sweep over the cluster finds every constraint within tolerance; at most max_iter
 * correcting sweeps are followed by one that only tests.  x, v and the velocity Dx / dt that S adds are each rounded to fp32 once,
 * after the iteration.  Fixed order, no atomics in the arithmetic, no dependence on the launch geometry: repeats are bit-identical,
 * as long as no cluster fails (below).
 * Failure: a cluster that has not converged, or that met a non-finite value, writes x_keep / v_keep of its atoms back to pos /
 * vel (PROJECT: leaves vel alone), ORs the fail word in cons_ws and does nothing else - unconverged positions are never written, the
 * evaluation that follows always sees finite coordinates.  The next reduction (PROJECT: a latch of its own) sets status 3, writes no
 * log row and does not advance the step counter; from then on every launch returns at once.  The state is then frozen and finite,
 * but not a point of the trajectory: other clusters may be half a step ahead.  Which ones is not reproducible: a cluster reads the
 * fail word when it starts, while other clusters of the same launch may be setting it, so the clusters of a failing launch that
 * still complete their half step depend on the scheduling, and the frozen state can differ from run to run.  To continue: zero cons_ws, tmdnet_md_reset, new
 * positions and velocities.  Overflow (status 1) is handled as by tmdnet_md_advance.
 *   cons_ws       tmdnet_md_constraints_workspace_bytes bytes, ZEROED by the caller before the first launch and with every
 *                 tmdnet_md_reset.
 *   md_ws, pos ... ekin_log_row   as in tmdnet_md_advance, but mass is read in every phase; forces, hk may be NULL for PROJECT.
 *   cluster_atoms    [n_clusters, 8] int32: the caller's atom indices, -1 = no atom; every atom exactly once.
 *   cluster_offsets  [n_clusters + 1] int32: the constraints of cluster c are rows cluster_offsets[c] .. cluster_offsets[c + 1] of
 *   constraint_ends  [n_constraints, 2] int32: the two ends as positions 0 .. 7 in the cluster's row of cluster_atoms, and
 *   constraint_d2    [n_constraints] double: d_c^2.
 *   tol > 0, max_iter >= 1. */
#define TMDNET_MD_PROJECT 3 /* tmdnet_md_advance_constrained only: R alone */
int tmdnet_md_constraints_workspace_bytes(int64_t n_atoms, int64_t n_clusters, int64_t n_constraints, size_t* bytes);
int tmdnet_md_advance_constrained(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* cons_ws, int64_t n_atoms,
                                  int64_t n_mol, int32_t phase, float* pos, float* vel, const float* forces, const float* energy,
                                  const float* hk, const float* mass, const float* sigma, float dt, float c1, float c2, uint64_t seed,
                                  const int64_t* batch, float* forces_keep, float* epot_log_row, float* ekin_log_row,
                                  int64_t n_clusters, int64_t n_constraints, const int32_t* cluster_atoms,
                                  const int32_t* cluster_offsets, const int32_t* constraint_ends, const double* constraint_d2, double tol,
                                  int32_t max_iter);

/* ---- Device-resident geometry minimisation (csrc/tn_min.hip; additive exports, the ABI revision stays 10) ---------------------
 * FIRE (Bitzek et al., Phys. Rev. Lett. 97, 170201, 2006) in the form ASE ships: unit masses, the whole-molecule step clamp, and
 * one controller per molecule (replica), so that every molecule of a batch has its own time step and converges at its own step.
 * The launches sit between two tmdnet_energy_forces calls of a captured step: K steps replay as one HIP graph.  The box is fixed.
 * Per step, from the forces F at the current positions (an atom with fixed[i] != 0 contributes nothing and never moves):
 *   per atom, fp32 under the rounding contract of the MD loop (one rounded product, one rounded sum, in this order):
 *     t_vf = (Fx vx + Fy vy) + Fz vz,  t_ff and t_vv likewise
 *   per molecule, the fp32 terms widened and added in fp64 in a fixed order (threads stride the atoms, a wave tree, waves in turn,
 *   slices in slice order; no floating-point atomics):  vf, ff, vv, fmax2 = max_i t_ff
 *   per molecule, one thread, fp64, in this order (`step` = steps completed, this one included):
 *     1. converged_at >= 0: nothing (the molecule stays frozen)
 *     2. a sum is not finite: status 2 (below)
 *     3. sqrt(fmax2) < fmax: converged_at = step, frozen
 *     4. vf > 0:  c_v = 1 - alpha;  mix = (ff > 0 && vv > 0) ? alpha sqrt(vv / ff) : 0;
 *                 n_pos > n_min: dt = min(dt f_inc, dt_max), alpha = alpha f_alpha;   n_pos += 1
 *     5. else:    c_v = 0, mix = 0, alpha = alpha0, dt = dt f_dec, n_pos = 0
 *     6. c_f = mix + dt                                      (the new dt)
 *     7. n2 = ((c_v c_v) vv + ((2 c_v) c_f) vf) + (c_f c_f) ff        (|v_new|^2 from the sums: the clamp needs no second reduction)
 *     8. len = dt sqrt(max(n2, 0));   d = len > max_step ? dt (max_step / len) : dt
 *     9. c_v, c_f, d rounded to fp32 once
 *   per atom, fp32 under the contract:  v <- (c_v v) + (c_f F),  x <- x + (d v);  frozen molecule or fixed atom: v <- 0 and x is
 *   not touched (a branch, not a product with 0).
 * Without a thermostat there is no noise: a minimisation is a fixed sequence of IEEE operations, bit-identical from run to run. */
#define TMDNET_MIN_OPEN 0   /* the per-atom update alone, from the coefficients the workspace holds (first launch of a replay) */
#define TMDNET_MIN_MIDDLE 1 /* after an evaluation: accept it, reduce, control, update */
#define TMDNET_MIN_CLOSE 2  /* after the last evaluation of a replay, and once after a reset: accept, reduce, control */
/* Bytes of the minimiser state `min_ws`: a 256-byte header (64-bit step counter, sticky status, the start values), per molecule
 * dt and alpha (fp64), n_pos (int32), converged_at (int64) and the three coefficients, the positions and velocities before the
 * last move (24 bytes per atom) and the slice sums (32 bytes per molecule and slice of at most 1 024 atoms on average). */
int tmdnet_min_workspace_bytes(int64_t n_atoms, int64_t n_mol, size_t* bytes);
/* Enqueues: step counter = step0, status = 0; every molecule restarts from dt0, alpha0, n_pos = 0, converged_at = -1 at the next
 * control.  After a reset the first launch must be tmdnet_min_advance(TMDNET_MIN_CLOSE) on the forces at the start geometry (with
 * vel = 0): it computes the first coefficients - a molecule already below fmax converges at step0 - and counts no step.  An
 * OPEN or MIDDLE launch's update before that does nothing. */
int tmdnet_min_reset(void* stream, void* min_ws, uint64_t step0, double dt0, double alpha0);
/* Enqueues one phase.  A replay of K steps is OPEN, then K times { evaluation at `pos`; MIDDLE, or CLOSE after the last }: every
 * evaluated force set drives the controller exactly once, whatever K is.  MIDDLE / CLOSE are three launches (the reduction on a
 * grid (n_mol, slices), the controller as one block, one thread per atom), OPEN is one.
 *   m, graph_ws   the handle and graph workspace of the evaluation before this launch: its overflow flag is read, and the atom
 *                 ranges of the molecules are taken from it when they are valid.  graph_ws == NULL (m may then be NULL): no
 *                 overflow test, the sums run over all atoms filtered by `batch` (NULL: one molecule).
 *   pos, vel      [n_atoms, 3], updated in place; vel is the minimiser's own velocity (zero at the start).
 *   forces        [n_atoms, 3], read only: the evaluation's output (MIDDLE / CLOSE) or the kept forces (OPEN).
 *   energy        [n_mol] or NULL: copied to epot_log_row.
 *   fixed         [n_atoms] bytes or NULL;  batch   [n_atoms] int64 molecule index in the caller's order, or NULL.
 *   forces_keep   [n_atoms, 3] or NULL: MIDDLE / CLOSE copy `forces` here once the step is accepted, so that a buffer the caller
 *                 owns holds the forces at `pos` after a CLOSE (the `forces` of the next replay's OPEN).
 *   dt_max ... fmax   the FIRE parameters above (dt0 and the first alpha are tmdnet_min_reset's); fmax > 0.
 *   log rows      each [n_mol] or NULL, of the force set just controlled: epot, fmax = sqrt(fmax2) as fp32, sums [n_mol, 4] fp64
 *                 (vf, ff, vv, fmax2), coef [n_mol, 3] fp32 (c_v, c_f, d of the NEXT move; 0 for a frozen molecule), dt and alpha
 *                 (fp64, after the update), converged_at (int64, -1: not yet).
 * Overflow: when the evaluation before a MIDDLE / CLOSE launch overflowed, the controller sets status 1 and pos and vel go back
 * to what the last move saved.  Status 2: a sum of a molecule that still moves was not finite (a NaN force); nothing of that step
 * is written.  Either way every later launch leaves pos, vel, forces_keep, the log rows, the controller state and the step counter
 * alone until tmdnet_min_reset. */
int tmdnet_min_advance(tmdnet_model* m, void* stream, void* graph_ws, void* min_ws, int64_t n_atoms, int64_t n_mol, int32_t phase,
                       float* pos, float* vel, const float* forces, const float* energy, const uint8_t* fixed, const int64_t* batch,
                       float* forces_keep, double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha0, double f_alpha,
                       double max_step, double fmax, float* epot_log_row, float* fmax_log_row, double* sums_log_row,
                       float* coef_log_row, double* dt_log_row, double* alpha_log_row, int64_t* converged_log_row);
/* host[0] = steps completed (the device counter), host[1] = status (1: an evaluation overflowed, 2: a non-finite force sum; the
 * state is that of step host[0]).  Synchronises the stream.  Returns TMDNET_ERR_OVERFLOW for status 1, TMDNET_ERR_STATE for 2. */
int tmdnet_min_status(void* stream, void* min_ws, uint64_t host[2]);

/* ---- Cell relaxation in the minimiser (csrc/tn_min.hip; additive exports, the ABI revision stays 10) ---------------------------
 * ASE's UnitCellFilter scheme on top of the controller above, one per molecule: the box relaxes together with the atoms.  Row
 * vectors, as for the virial.  State per molecule, fp64: the reference box H0 (the box at the reset), the deformation gradient D
 * (I at the reset), its FIRE velocity V_D, c = cell_factor.  The box the evaluation reads is H = H0 D^T, its nine entries rounded to
 * fp32 once; D32 = fp32(D).  State per atom, fp32: xt = x D^-T and its velocity vt; the position handed to the evaluation is
 *     x_a = (xt_0 D32[a][0] + xt_1 D32[a][1]) + xt_2 D32[a][2]            (each product one rounded product, each sum one rounded sum)
 * Generalised forces, with the D32 the positions were formed with:
 *     atoms   Ft_b = (F_0 D32[0][b] + F_1 D32[1][b]) + F_2 D32[2][b]
 *     cell    W_s = (W + W^T) / 2 from the step's virial;  V = |det box| of the fp32 box the evaluation read;
 *             G = (W_s - pressure V I) D^-T  (D^-1 by cofactors);  = - d(E + pressure V) / dD at fixed xt
 *             hydrostatic: G <- (tr G / 3) I;  constant_volume: G <- G - (tr G / 3) I;  then G <- mask o G, entry by entry
 *     the three rows of G / c count as three more atoms with coordinates c D and velocity V_D.
 * The sums vf, ff, vv, fmax2 of the atoms (from Ft and vt, reduced as above) get the three rows' fp64 terms added in the controller,
 * so the convergence test and the max_step clamp see all N + 3 rows.  The controller is the one above; with its three fp32
 * coefficients, widened, V_D <- c_v V_D + c_f G / c and D <- D + (d V_D) / c in fp64, and per atom vt <- c_v vt + c_f Ft,
 * xt <- xt + d vt, x from the new D32.  A converged molecule changes neither D nor the box nor its atoms; a fixed atom has vt = 0,
 * contributes to no sum and keeps xt, so it follows the cell affinely.  With mask = 0, D stays I and every product with D32 is exact:
 * the run equals tmdnet_min_advance bit for bit.
 * Status 2 is also latched, before anything of the step is written, for a virial entry that is not finite and for a box whose
 * volume is zero (now, or after the move about to be made); tmdnet_min_status_cell says which.  The move saves xt, vt and per
 * molecule D, V_D and the fp32 box; an overflowing evaluation puts all of them, the box and pos back (status 1). */
/* bytes of `min_ws` for the entries below: tmdnet_min_workspace_bytes plus 540 bytes per molecule (ten arrays, each rounded up to 256 bytes) */
int tmdnet_min_workspace_bytes_cell(int64_t n_atoms, int64_t n_mol, size_t* bytes);
/* tmdnet_min_reset, and per molecule H0 = box, D = I, V_D = 0; per atom xt = pos.  box [n_mol, 9] fp32, deform and cell_vel
 * [n_mol, 9] fp64, pos and xt [n_atoms, 3]. */
int tmdnet_min_reset_cell(void* stream, void* min_ws, int64_t n_atoms, int64_t n_mol, uint64_t step0, double dt0, double alpha0,
                          const float* box, double* deform, double* cell_vel, const float* pos, float* xt);
/* tmdnet_min_advance - its 29 arguments in its order, with its meaning, but `vel` is vt and `pos` is written from xt - plus:
 *   xt            [n_atoms, 3] the integrated coordinates.
 *   box           [n_mol, 9] the box the evaluations read: rewritten by every move.
 *   deform, cell_vel   [n_mol, 9] fp64: D and V_D.
 *   virial        [n_mol, 9] of the evaluation before this launch (MIDDLE / CLOSE; may be NULL for OPEN).
 *   cell_factor   [n_mol] fp64, each > 0.
 *   mask          nine doubles on the HOST, read before the call returns: 0 drops the entry of G.
 *   flags         bit 0 hydrostatic, bit 1 constant_volume (not both);  pressure in E / length^3.
 *   log rows      stress [n_mol, 9] fp64 = -W_s / V, volume [n_mol] fp64, cell_force [n_mol, 9] fp64 = G / c; each may be NULL.
 * The fmax log row includes the cell rows; the sums log row holds the atoms' sums (of Ft and vt), to which the controller adds the
 * cell rows' terms from cell_force and V_D.  OPEN is two launches (the cell's part of the move, then the atoms). */
int tmdnet_min_advance_cell(tmdnet_model* m, void* stream, void* graph_ws, void* min_ws, int64_t n_atoms, int64_t n_mol, int32_t phase,
                            float* pos, float* vel, const float* forces, const float* energy, const uint8_t* fixed, const int64_t* batch,
                            float* forces_keep, double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha0, double f_alpha,
                            double max_step, double fmax, float* epot_log_row, float* fmax_log_row, double* sums_log_row,
                            float* coef_log_row, double* dt_log_row, double* alpha_log_row, int64_t* converged_log_row, float* xt,
                            float* box, double* deform, double* cell_vel, const float* virial, const double* cell_factor,
                            const double* mask, int32_t flags, double pressure, double* stress_log_row, double* volume_log_row,
                            double* cell_force_log_row);
/* tmdnet_min_status, and host[2] = what was unusable when status is 2: 1 a force sum, 2 the virial, 3 the volume of the box. */
int tmdnet_min_status_cell(void* stream, void* min_ws, uint64_t host[3]);

/* ---- L-BFGS in the device-resident minimiser (csrc/tn_lbfgs.hip; additive exports, the ABI revision stays 10) -------------------
 * ASE's LBFGS without line search, one optimiser per molecule (replica): each has its own history and converges at its own step;
 * the freezing rules are those of the FIRE entries above.  Parameters: memory (pairs held, 1 .. 512), alpha (H0 = 1 / alpha),
 * max_step, damping.  The box is fixed.  With g = -F, per molecule and step (an atom with fixed[i] != 0 contributes nothing and never
 * moves):
 *   1. after a move, the candidate pair s = x - x_prev, y = F_prev - F, each component one rounded fp32 subtraction.  It enters the
 *      history only when s.y > 0; when the history holds `memory` pairs the oldest leaves.  (ASE stores every pair and can divide by
 *      zero or step uphill: dropping a pair that violates the curvature condition is the one deviation.  Where every pair passes, the
 *      sequence is ASE's.)
 *   2. the two-loop recursion: q = g; newest ... oldest: a_i = (s_i.q) / (y_i.s_i), q -= a_i y_i; z = q / alpha; oldest ... newest:
 *      b = (y_i.z) / (y_i.s_i), z += s_i (a_i - b); p = -z.  It runs in fp64 on the coefficients of q and z in the basis (s_j, y_j, g),
 *      given the Gram matrix of that basis: the scalar products are sums of exact fp64 products of widened fp32 values in a fixed
 *      order (lanes stride the atoms, a wave tree, slices in slice order; no floating-point atomics).
 *   3. per atom p_i = -(delta_g g_i + sum over the pairs, oldest first, (delta_s s_i + delta_y y_i)) in fp64, rounded to fp32 once
 *   4. ASE's clamp for this class is per ATOM: longest = max_i |p_i| (fp64, of the rounded p); c = damping (longest >= max_step ?
 *      max_step / longest : 1), rounded to fp32 once;  x <- x + (c p), one rounded product and one rounded sum
 *   5. a molecule converges when sqrt(max_i |F_i|^2) < fmax and is then frozen: x is not touched (a branch, not a product with 0).
 * A minimisation is a fixed sequence of IEEE operations, bit-identical from run to run. */
/* Bytes of the L-BFGS state `lbfgs_ws`: a 256-byte header (64-bit step counter, sticky status, its cause); per atom x_prev and F_prev
 * (24 bytes, also what an overflow restores) and the rings S and Y as fp32 [memory + 1][n_atoms][3] (24 (memory + 1) bytes: the extra
 * slot holds the candidate, so a rejected candidate overwrites nothing); per molecule the pairs held, the ring order, converged_at,
 * the three Gram blocks SS, SY, YY in fp64 by slot (24 (memory + 1)^2 bytes), the coefficients of the move prepared and the sums
 * (64 (memory + 1) bytes, and 48 (memory + 1) per slice of at most 1 024 atoms on average).  A caller with thousands of small
 * molecules picks a smaller memory.  memory < 1 or > 512: TMDNET_ERR_INVALID. */
int tmdnet_lbfgs_workspace_bytes(int64_t n_atoms, int64_t n_mol, int32_t memory, size_t* bytes);
/* Where the state lies, for a caller that wants to read it: byte offsets from the workspace pointer rounded up to 256 of
 * [0] the header, [1] pairs held int32 [n_mol], [2] converged_at int64 [n_mol], [3] the ring order int32 [n_mol, memory + 1] (entries
 * 0 .. h - 1: the slots held, oldest first; entry h: the spare slot, which holds the last candidate), [4] SS, [5] SY, [6] YY fp64
 * [n_mol, memory + 1, memory + 1] by slot, [7] the coefficients fp64 [n_mol, 2 (memory + 1) + 1] (s by slot, y by slot, g), [8] the
 * sums, [9] the slice sums, [10] the slice maxima of |p_i|^2, [11] x_prev, [12] F_prev fp32 [n_atoms, 3], [13] S, [14] Y fp32
 * [memory + 1, n_atoms, 3], [15] the clamp factor of the last move fp32 [n_mol], [16] the end. */
int tmdnet_lbfgs_layout(int64_t n_atoms, int64_t n_mol, int32_t memory, int64_t offsets[17]);
/* Enqueues: step counter = step0, status = 0; the next control empties every molecule's history and sets converged_at = -1.  After a
 * reset the first launch must be tmdnet_lbfgs_advance(TMDNET_MIN_CLOSE) on the forces at the start geometry: h = 0, p = F / alpha, a
 * molecule already below fmax converges at step0, and no step is counted.  An OPEN launch before that does nothing. */
int tmdnet_lbfgs_reset(void* stream, void* lbfgs_ws, uint64_t step0);
/* Enqueues one phase, with the meaning of TMDNET_MIN_OPEN / MIDDLE / CLOSE above: a replay of K steps is OPEN, then K times
 * { evaluation at `pos`; MIDDLE, or CLOSE after the last }.  MIDDLE is four launches - the scalar products on a grid (n_mol, slices),
 * the controller with one wave per molecule, the direction on the same grid, one thread per atom for the move -,
 * CLOSE the same four with a last one that only accepts the evaluation, OPEN the move alone: 4 K + 1 launches per replay.
 *   m, graph_ws   as tmdnet_min_advance: the overflow flag and the atom ranges of the evaluation before this launch; both may be NULL
 *                 (no overflow test, atoms filtered by `batch`).
 *   pos           [n_atoms, 3], updated in place.   forces   [n_atoms, 3], read only: the evaluation's output (MIDDLE / CLOSE) or the
 *                 kept forces (OPEN).   energy   [n_mol] or NULL: copied to epot_log_row.
 *   fixed         [n_atoms] bytes or NULL;  batch   [n_atoms] int64 molecule index in the caller's order, or NULL (one molecule).
 *   forces_keep   [n_atoms, 3] or NULL: MIDDLE / CLOSE copy `forces` here once the step is accepted.
 *   direction     [n_atoms, 3], the caller's: p of the move prepared (0 for a fixed atom; not rewritten once a molecule is frozen).
 *   memory ... fmax   the parameters above; the same memory as in tmdnet_lbfgs_workspace_bytes.
 *   log rows      each [n_mol] or NULL, of the force set just controlled: epot, fmax = sqrt(fmax2) as fp32, sums [n_mol, 4] fp64 (ff,
 *                 fmax2, s_c.y_c of the candidate (0: there was none), g.p of the move prepared, from the coefficients), pairs held
 *                 (int32), accepted (int32: 1 when the candidate entered the history), scale (fp32: the clamp factor c of the move
 *                 that LED to this force set, which the move kept in the workspace; 0 for the start geometry and for a molecule
 *                 that was frozen), converged_at (int64, -1: not yet).
 * Overflow: when the evaluation before a MIDDLE / CLOSE launch overflowed, the controller sets status 1 and pos goes back to x_prev;
 * the history is intact, because the candidate sat in the spare slot.  Status 2: a sum of a molecule that still moves was not finite;
 * nothing of that step is written.  Either way every later launch leaves pos, forces_keep, direction, the log rows, the history and
 * the step counter alone until tmdnet_lbfgs_reset. */
int tmdnet_lbfgs_advance(tmdnet_model* m, void* stream, void* graph_ws, void* lbfgs_ws, int64_t n_atoms, int64_t n_mol, int32_t phase,
                         float* pos, const float* forces, const float* energy, const uint8_t* fixed, const int64_t* batch,
                         float* forces_keep, float* direction, int32_t memory, double alpha, double max_step, double damping, double fmax,
                         float* epot_log_row, float* fmax_log_row, double* sums_log_row, int32_t* pairs_log_row,
                         int32_t* accepted_log_row, float* scale_log_row, int64_t* converged_log_row);
/* tmdnet_min_status on the L-BFGS state, and host[2] = what was unusable when status is 2 (1: a sum). */
int tmdnet_lbfgs_status(void* stream, void* lbfgs_ws, uint64_t host[3]);

/* ---- Device-resident nudged elastic band (csrc/tn_neb.hip; additive exports, the ABI revision stays 10) ------------------------
 * A minimum-energy path and its saddle point: NEB with the improved tangent (Henkelman and Jonsson, J. Chem. Phys. 113, 9978, 2000)
 * and a climbing image, driven by the FIRE controller above with ONE controller per band.  The launches sit between two
 * tmdnet_energy_forces calls of a captured step: K band steps replay as one HIP graph.
 * Storage: a band has M >= 3 images of the same n atoms, a call has G >= 1 bands; rows are image-major, atom a of image i of band g
 * is row (g M + i) n + a, and the evaluation sees G M molecules of n atoms.  Images 0 and M - 1 of every band never move (a branch:
 * their positions keep their bits); they are evaluated with the rest and their energies feed the tangents.  No minimum image is
 * applied between images: the caller supplies an unwrapped path.
 * Per step, for every interior image i, from the energies E and forces F at the current positions:
 *   per atom, fp32 under the rounding contract of the MD loop:  d+ = R_{i+1} - R_i,  d- = R_i - R_{i-1}  (one rounded sum per
 *     component), and the terms  d+.d+, d-.d-, d+.d-, F.d+, F.d-  each as (x + y) + z of three rounded products; an atom with
 *     fixed[a] != 0 contributes nothing
 *   per image, the terms widened and added in fp64 in the fixed order of the minimiser's sums:  a, b, c, p, q
 *   per image, fp64, from the fp32 energies widened - the improved tangent tau = w+ d+ + w- d-:
 *     E_{i+1} > E_i > E_{i-1}: (w+, w-) = (1, 0);   E_{i+1} < E_i < E_{i-1}: (0, 1);   otherwise hi / lo = the larger / smaller of
 *     |E_{i+1} - E_i| and |E_{i-1} - E_i|, and (w+, w-) = (hi, lo) when E_{i+1} > E_{i-1}, else (lo, hi)
 *     |tau|^2 = ((w+ w+) a + ((2 w+) w-) c) + (w- w-) b;   F.tau = w+ p + w- q
 *     g = (-(F.tau / |tau|) + k (sqrt a - sqrt b)) / |tau|       (F - (F.tau^) tau^ + k (|d+| - |d-|) tau^; k = spring_k, E / length^2)
 *     the climber, when climbing is on: g = (-2 F.tau) / |tau|^2  (F - 2 (F.tau^) tau^, no spring).  The climber of a band is the
 *     lowest interior index with the largest energy, chosen anew at every step from that step's energies.
 *     s+ = fp32(g w+), s- = fp32(g w-), each rounded once
 *   per atom, fp32 under the contract:  F_neb = (F + s+ d+) + s- d-;  a fixed atom keeps F, an endpoint image has F_neb = 0
 *   per band: vf, ff, vv, fmax2 of the minimiser over all interior images on F_neb (per image in the minimiser's order, the images
 *     added in image order), then the minimiser's controller, unchanged: the band converges when sqrt(fmax2) < fmax and freezes then,
 *     and the max_step clamp acts on the whole band's move
 *   per atom the minimiser's update with the band's three coefficients; fixed atoms, endpoint images and frozen bands: v <- 0, x
 *     is not touched.
 * A band that still moves is unusable - status 2, nothing of that step is written - when an energy of the band is not finite
 * (cause 3), when |tau|^2 of an image is zero or not finite (cause 2: coincident images), or when F.tau or a FIRE sum is not
 * finite (cause 1).  When every atom is fixed no image has a degree of freedom: no tangent is formed, nothing is unusable and the
 * band converges as it stands.  Overflow is the minimiser's protocol: the move saves x and v, an overflowed evaluation latches status 1 and
 * puts them back.  Only the single-block controller writes the status word; every later launch returns at once until a reset. */
/* Bytes of the band state `neb_ws`: a 256-byte header (step counter, status, the start values, the climb flag, the cause), per band
 * the controller's state and coefficients, per image its path sums, weights, coefficients and the slice sums, per row the position
 * and velocity before the last move and F_neb (36 bytes).  n_images >= 3, n_bands >= 1. */
int tmdnet_neb_workspace_bytes(int64_t n_atoms_per_image, int64_t n_images, int64_t n_bands, size_t* bytes);
/* tmdnet_min_reset, and climb = 1 / 0 switches the climbing image on / off for every band: one captured graph serves the plain phase
 * and the climbing phase.  The first launch after it must be tmdnet_neb_advance(TMDNET_MIN_CLOSE) on the start path (vel = 0). */
int tmdnet_neb_reset(void* stream, void* neb_ws, uint64_t step0, double dt0, double alpha0, int32_t climb);
/* Enqueues one phase (TMDNET_MIN_OPEN / MIDDLE / CLOSE with the minimiser's meaning).  MIDDLE and CLOSE are four launches - the path
 * sums on a grid (image, slice); the projection on the same grid, every block deriving its image's coefficients from the slice sums;
 * the controller as one block; one thread per row - and OPEN is one.  The arguments of tmdnet_min_advance with its meaning, except:
 *   n_atoms_per_image, n_images, n_bands   replace n_atoms, n_mol and batch (the evaluation had n_images n_bands molecules).
 *   forces        MIDDLE / CLOSE: the evaluation's F;  OPEN: the kept F_neb.
 *   energy        [n_bands, n_images], required for MIDDLE / CLOSE.
 *   fixed         [n_atoms_per_image] bytes or NULL: the same atoms in every image.
 *   forces_keep   receives F_neb once the step is accepted.
 *   spring_k      > 0, after fmax.
 *   log rows      epot [n_bands, n_images]; fmax, sums, coef, dt, alpha, converged_at per BAND as for the minimiser; then per image
 *                 path_sums [n_bands, n_images, 5] fp64 (a, b, c, p, q), weights [.., 2] fp64 (w+, w-), tangent_coef [.., 2] fp32
 *                 (s+, s-), zero on endpoints; and climber [n_bands] int32, the interior image with the largest energy (the image
 *                 that climbs when climbing is on).  Each may be NULL. */
int tmdnet_neb_advance(tmdnet_model* m, void* stream, void* graph_ws, void* neb_ws, int64_t n_atoms_per_image, int64_t n_images,
                       int64_t n_bands, int32_t phase, float* pos, float* vel, const float* forces, const float* energy,
                       const uint8_t* fixed, float* forces_keep, double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha0,
                       double f_alpha, double max_step, double fmax, double spring_k, float* epot_log_row, float* fmax_log_row,
                       double* sums_log_row, float* coef_log_row, double* dt_log_row, double* alpha_log_row,
                       int64_t* converged_log_row, double* path_sums_log_row, double* weights_log_row, float* tangent_coef_log_row,
                       int32_t* climber_log_row);
/* tmdnet_min_status, and host[2] = what was unusable when status is 2: 1 a force sum, 2 the path (coincident images), 3 an energy. */
int tmdnet_neb_status(void* stream, void* neb_ws, uint64_t host[3]);

/* ---- Device-resident dimer saddle search (csrc/tn_dimer.hip; additive exports, the ABI revision stays 10) ------------------------
 * A first-order saddle from ONE known state by minimum-mode following: the dimer method (Henkelman and Jonsson, J. Chem. Phys. 111,
 * 7010, 1999) with forward differences (Heyden, Bell and Keil, J. Chem. Phys. 123, 224101, 2005) and the rotation from two curvature
 * rows (Kaestner and Sherwood, J. Chem. Phys. 128, 014106, 2008), driven by the FIRE controller above with ONE controller per dimer.
 * The launches sit between two tmdnet_energy_forces calls of a captured step: K steps replay as one HIP graph.
 * Storage: a call has G >= 1 dimers of the same n atoms.  A dimer carries its midpoint R0, a unit axis N and a unit partner
 * direction M at a right angle to N, both fp32 [n, 3] and zero on fixed atoms (mode, partner [G, n, 3]).  Every step evaluates three
 * images as one batch of 3 G molecules, rows image-major: atom a of image i of dimer g is row (g 3 + i) n + a, with image 0 = R0,
 * image 1 = R0 + delta N, image 2 = R0 + delta M (no minimum image between images).  vel, the kept forces, mode and partner have
 * one row per atom of a DIMER: [G, n, 3].
 * Per step, from the energies E and the forces F0, F1, F2 of the three images, dl = fp32(delta), inv = fp32(1 / delta):
 *   per atom, fp32 under the rounding contract of the MD loop:  HN = (F0 - F1) inv,  HM = (F0 - F2) inv  (one rounded sum, one
 *     rounded product per component), and the terms N.HN, N.HM, M.HN, M.HM, F0.N, F0.M each as (x + y) + z of three rounded
 *     products, and (F0.F0 + F1.F1) + F2.F2; an atom with fixed[a] != 0 contributes nothing
 *   per dimer, the terms widened and added in fp64 in the fixed order of the minimiser's sums; then, fp64 in the order written:
 *     a = N.HN,  b = (N.HM + M.HN) / 2,  c = M.HM
 *     (co, si), co >= 0, the unit eigenvector of [[a, b], [b, c]] for the smaller eigenvalue:  b = 0: (1, 0) when a <= c (the tie
 *     a = c keeps the axis), (0, 1) when a > c;  otherwise theta = atan2(-2 b, c - a) / 2, co = cos theta, si = sin theta
 *     nu^2 = sum over the free atoms of |co N + si M|^2, from the vectors, every term in fp64;  nu = sqrt(nu^2)
 *     C = (((co co) a + ((2 co) si) b) + (si si) c) / nu^2        (the curvature N'.HN' along the new axis)
 *     p = (co F0.N + si F0.M) / nu                                 (F0.N')
 *     cn = fp32(co / nu), sn = fp32(si / nu), cc = fp32(C);  C < 0: k0 = 1, e = fp32(-2 p);  otherwise k0 = 0, e = fp32(-p)
 *   per atom, fp32 under the contract:  N' = cn N + sn M,  HN' = cn HN + sn HM,  T = HN' - cc N' (the rotation residual),
 *     R = -fp32(si) N + fp32(co) M (the rotated partner),  F_eff = k0 F0 + e N'  - that is F0 - 2 (F0.N') N' where the curvature is
 *     negative and -(F0.N') N' in the convex region (Henkelman's rule); a fixed atom has N' = T = 0 and keeps F0
 *   per dimer: vf, ff, vv, fmax2 of the minimiser on F_eff over the free atoms of image 0, and T.T, T.N', N'.N', R.R, R.N', HN'.HN';
 *     the next partner M' = (mt T + mr R) + mn N':  k = T.N' / N'.N',  |T_perp|^2 = T.T - k T.N'  (T made orthogonal to N'),
 *     mt = fp32(1 / |T_perp|), mn = fp32(-(k / |T_perp|)), mr = 0 - unless |T_perp|^2 is zero, not finite or at most 2^-40 HN'.HN':
 *     then R takes T's place (mt = 0; mr, mn likewise from R.R and R.N'), so a converged mode keeps a defined partner; M' = 0 when R
 *     has no length either.  |T| = sqrt(T.T) is logged; with forward differences it does not go to zero and is no criterion.
 *     Then the minimiser's controller, unchanged, with the dimer's sums: the dimer converges when sqrt(fmax2) < fmax AND C < 0
 *     (while C >= 0 the controller is handed a bound of zero) and is frozen bit for bit from then on - R0, N, M and the kept forces.
 *   per atom: N <- N', M <- M', the minimiser's update of R0 with the dimer's three coefficients on F_eff (fixed atoms and frozen
 *     dimers: v <- 0, x is not touched), then - at every launch - image 1 <- R0 + dl N and image 2 <- R0 + dl M, each one rounded
 *     product and sum.
 * translate = 0 (tmdnet_dimer_reset) is a mode search: R0 keeps its bits, the FIRE state is not touched, no dimer converges, and
 * the loop only refines N and C.
 * A dimer that still moves is unusable - status 2, nothing of that step is accepted - when an energy of its three images is not
 * finite (cause 3), when a force sum or a FIRE sum is not finite (cause 1), or when a, b, c or nu^2 is not finite or nu^2 is zero
 * (cause 2: the mode has no length).  When every atom is fixed there is no mode: nothing is unusable and the dimer converges as it
 * stands.  Overflow is the minimiser's protocol: the move saves R0 and v, an overflowed evaluation latches status 1 and puts them
 * back (and rewrites the images from them).  Only the single-block controller writes the status word; every later launch returns
 * at once until a reset. */
/* Bytes of the dimer state `dimer_ws`: a 256-byte header (step counter, status, the start values, the translate flag, the cause),
 * per dimer the controller's state, the coefficients, the sums and the slice sums, per atom of a dimer R0 and v before the last
 * move and the pending F_eff, N' and T (60 bytes).  n_dimers >= 1. */
int tmdnet_dimer_workspace_bytes(int64_t n_atoms_per_image, int64_t n_dimers, size_t* bytes);
/* tmdnet_min_reset, and translate = 1 / 0 switches the move of the midpoint on / off for every dimer: one captured graph serves the
 * saddle search and the mode search.  The first launch after it must be tmdnet_dimer_advance(TMDNET_MIN_CLOSE) on the start
 * images (vel = 0; images 1 and 2 written by the caller as R0 + fp32(delta) N, R0 + fp32(delta) M). */
int tmdnet_dimer_reset(void* stream, void* dimer_ws, uint64_t step0, double dt0, double alpha0, int32_t translate);
/* Enqueues one phase (TMDNET_MIN_OPEN / MIDDLE / CLOSE with the minimiser's meaning).  MIDDLE and CLOSE are four launches - the
 * sums on a grid (dimer, slice of <= 1 024 atoms); the projection on the same grid, every block deriving its dimer's rotation from
 * the slice sums; the controller as one block; one thread per atom of a dimer for its three rows - and OPEN is one.  The arguments
 * of tmdnet_neb_advance with its meaning, except:
 *   n_atoms_per_image, n_dimers   the evaluation had 3 n_dimers molecules;  pos [3 n_dimers n, 3],  vel [n_dimers n, 3].
 *   mode, partner [n_dimers, n, 3]   N and M, read and rewritten.
 *   forces        MIDDLE / CLOSE: the evaluation's F [3 n_dimers n, 3];  OPEN: the kept F_eff [n_dimers n, 3].
 *   energy        [n_dimers, 3], required for MIDDLE / CLOSE.
 *   forces_keep, true_forces_keep [n_dimers n, 3]   receive F_eff and F0 once the step is accepted; each may be NULL.
 *   delta         > 0, in place of spring_k.
 *   log rows      epot [n_dimers] (image 0); fmax, sums, coef, dt, alpha, converged_at per DIMER as for the minimiser; then
 *                 curvature [n_dimers] fp64 (C), rotation [.., 2] fp64 (co, si), residual [n_dimers] fp64 (|T|), quad [.., 3] fp64
 *                 (a, b, c), mode_sums [.., 15] fp64 (N.HN, N.HM, M.HN, M.HM, F0.N, F0.M, the forces' squares, the number of free
 *                 atoms, nu^2, T.T, T.N', N'.N', R.R, R.N', HN'.HN') and mode_coef [.., 10] fp32 (cn, sn, cc, k0, e, fp32(co),
 *                 fp32(si), mt, mr, mn).  Each may be NULL. */
int tmdnet_dimer_advance(tmdnet_model* m, void* stream, void* graph_ws, void* dimer_ws, int64_t n_atoms_per_image, int64_t n_dimers,
                         int32_t phase, float* pos, float* vel, float* mode, float* partner, const float* forces, const float* energy,
                         const uint8_t* fixed, float* forces_keep, float* true_forces_keep, double dt_max, int32_t n_min, double f_inc,
                         double f_dec, double alpha0, double f_alpha, double max_step, double fmax, double delta, float* epot_log_row,
                         float* fmax_log_row, double* sums_log_row, float* coef_log_row, double* dt_log_row, double* alpha_log_row,
                         int64_t* converged_log_row, double* curvature_log_row, double* rotation_log_row, double* residual_log_row,
                         double* quad_log_row, double* mode_sums_log_row, float* mode_coef_log_row);
/* tmdnet_min_status, and host[2] = what was unusable when status is 2: 1 a force or FIRE sum, 2 the mode, 3 an energy. */
int tmdnet_dimer_status(void* stream, void* dimer_ws, uint64_t host[3]);

/* ---- Device-resident intrinsic reaction coordinate (csrc/tn_irc.hip; additive exports, the ABI revision stays 10) ----------------
 * The path of steepest descent in mass-weighted coordinates from a saddle point, in both directions: the damped velocity Verlet
 * path follower of Hratchian and Schlegel (J. Phys. Chem. A 106, 165, 2002) - a classical trajectory with a = force_scale F / m
 * whose speed is put back to a constant v0 after every step, so that dx/dt is parallel to F / m; one evaluation per step, one time
 * step per path chosen from an error estimate.  The launches sit between two tmdnet_energy_forces calls of a captured step: K steps
 * replay as one HIP graph.
 * Storage: a call has G >= 1 saddles of the same n atoms and D = 1 or 2 directions; the P = G D paths are evaluated as one batch of
 * P molecules, rows path-major: atom a of path p = g D + d is row p n + a, with sigma = +1 for d = 0 (forward) and -1 for d = 1.
 * pos, vel and the kept forces are [P, n, 3]; half_inv_mass [n] holds c_a = fp32(force_scale / (2 m_a)) and masses [n] fp32(m_a).
 * An atom with fixed[a] != 0 or c_a = 0 (infinite mass) never moves, has v = 0 and is left out of every sum.
 * Start (the caller writes it): x_0 = x_TS + (sigma fp32(initial_step)) u and v_0 = (sigma fp32(v0)) u with u the unit direction,
 * zero on the atoms that never move; one rounded product (and sum) per component.
 * Step i -> i+1, with dt_i the path's time step rounded to fp32 once:
 *   open, before the evaluation (tn_md::open_step, unchanged):  hk = dt_i c_a,  v_half = v_i + hk F_i,  x_{i+1} = x_i + dt_i v_half;
 *     (x_i, v_i, F_i) is kept as generation 1 and the former generation 1 becomes generation 2: (x_{i-1}, v_{i-1}, F_{i-1}, dt_{i-1})
 *   per atom after the evaluation at x_{i+1}, fp32 under the rounding contract of the MD loop:  v' = v_half + hk F_{i+1}
 *   per path over the atoms that move, the fp32 terms widened and added in fp64 in the fixed order of the minimiser's sums:
 *     vv = sum |v'|^2,  P = sum F_{i+1}.v',  fmax2 = max |F_{i+1}|^2,  ds2 = sum m_a |x_{i+1} - x_i|^2,  the number of atoms, and -
 *     only when a generation 2 exists -  D2 = sum |x_{i+1} - x'|^2  with  x' = (x_{i-1} + T v_{i-1}) + (T T) (c_a F_{i-1}),
 *     T = dt_{i-1} + dt_i in fp32: where constant acceleration from two steps back would have led
 *   per path, fp64 in the order written:
 *     c = v0 / sqrt(vv)                                                                  (the damping; fp32(c) multiplies)
 *     dt_{i+1} = clamp(dt_i clamp(cbrt(error / sqrt(D2)), 1/2, 2), dt_min, dt_max); unchanged on a path's first step and when D2 = 0
 *     s_{i+1} = s_i + sqrt(ds2)                                                          (the mass-weighted arc length)
 *     the path finishes at this step when sqrt(fmax2) < fmax (reason 1), otherwise when P <= 0 (reason 2: it has turned uphill, the
 *     minimum lies within one step behind it), and is frozen bit for bit from then on - x, v, the kept forces, dt
 *   per atom:  v_{i+1} = fp32(c) v', one product; then the open of the next step.
 * The control of the start images (the launch after tmdnet_irc_reset) is the same with hk = 0, ds2 = 0 and the time step unchanged.
 * A path that still moves is unusable - status 2, nothing of that step is accepted and x, v of generation 1 are put back - when its
 * energy is not finite (cause 3), when P or fmax2 is not finite (cause 1), or when vv is zero or not finite or D2 or ds2 is not finite
 * (cause 2), looked at in this order.  When no atom of a path moves nothing is unusable and the path is finished as it stands.
 * Overflow is the minimiser's protocol: an overflowed evaluation latches status 1 and generation 1 is put back.  Only the
 * single-block controller writes the status word; every later launch changes nothing until a reset.
 * The path record lives in the workspace: on every `every`-th accepted step of a path (the start images are step 0) and on its
 * finishing step x_{i+1} is copied into the path's next frame, with s and the energy; when the `capacity` frames are full recording
 * stops and the count goes on counting.  Layout, so that a caller can read it: the workspace is used from its first address that is
 * a multiple of 256; the 256-byte header is followed by n_recorded int32 [P], frame_s fp64 [P, capacity], frame_energy fp32
 * [P, capacity] and frames fp32 [P, capacity, n, 3], each array beginning on the next multiple of 256 bytes. */
/* Bytes of the state `irc_ws`: the header (step counter, status, cause, the start time step), the record, per path the controller's
 * state, the sums and the slice sums, and per atom the two generations (72 bytes).  n_paths >= 1, capacity >= 1. */
int tmdnet_irc_workspace_bytes(int64_t n_atoms, int64_t n_paths, int64_t capacity, size_t* bytes);
/* Step counter = step0, status cleared, every path moving again with time step dt0 > 0, s = 0 and an empty record; both
 * generations are forgotten.  The first launch after it must be tmdnet_irc_advance(TMDNET_MIN_CLOSE) on the start images. */
int tmdnet_irc_reset(void* stream, void* irc_ws, uint64_t step0, double dt0);
/* Enqueues one phase (TMDNET_MIN_OPEN / MIDDLE / CLOSE with the minimiser's meaning).  MIDDLE and CLOSE are three launches - the
 * six sums in one pass on a grid (path, slice of <= 1 024 atoms); the controller as one block; one thread per atom - and OPEN is
 * one.  Nothing allocates or synchronises.
 *   m, graph_ws   as for tmdnet_min_advance (both NULL: no overflow counter is looked at).
 *   n_atoms, n_paths, capacity   as given to tmdnet_irc_workspace_bytes;  every >= 1.
 *   pos, vel [n_paths n, 3]   read and rewritten.
 *   forces        MIDDLE / CLOSE: the evaluation's F [n_paths n, 3];  OPEN: the kept forces.
 *   energy        [n_paths], required for MIDDLE / CLOSE.
 *   half_inv_mass, masses [n]; fixed [n] or NULL.
 *   forces_keep [n_paths n, 3]   receives F once the step is accepted; may be NULL.
 *   fmax, v0, error, dt_min <= dt_max   all > 0.
 *   log rows      epot, fmax [n_paths] fp32; sums [.., 6] fp64 (vv, P, fmax2, D2, ds2, the number of atoms that move); coef [.., 2]
 *                 fp32 (fp32(c), fp32(dt_i)); dt (dt_{i+1}), arc (s_{i+1}), power (P) [n_paths] fp64.  Each may be NULL.
 *   converged_at int64, reason int32, step_size fp64, arc_length fp64, n_recorded int32 [n_paths]   the paths' state after this
 *                 step.  Each may be NULL. */
int tmdnet_irc_advance(tmdnet_model* m, void* stream, void* graph_ws, void* irc_ws, int64_t n_atoms, int64_t n_paths, int64_t capacity,
                       int32_t every, int32_t phase, float* pos, float* vel, const float* forces, const float* energy,
                       const float* half_inv_mass, const float* masses, const uint8_t* fixed, float* forces_keep, double fmax, double v0,
                       double error, double dt_min, double dt_max, float* epot_log_row, float* fmax_log_row, double* sums_log_row,
                       float* coef_log_row, double* dt_log_row, double* arc_log_row, double* power_log_row, int64_t* converged_at,
                       int32_t* reason, double* step_size, double* arc_length, int32_t* n_recorded);
/* tmdnet_min_status, and host[2] = what was unusable when status is 2: 1 the forces, 2 the velocity or a path sum, 3 an energy. */
int tmdnet_irc_status(void* stream, void* irc_ws, uint64_t host[3]);

/* ---- Relaxed coordinate scans: a constrained FIRE minimiser in one graph (csrc/tn_scan.hip; additive exports, the ABI revision stays 10) ----
 * G points, each a copy of the same n atoms (atom a of point g is row g n + a; the evaluation sees G molecules), share D <= 4
 * collective variables - distance, angle, torsion, the functions and gradients of the MD bias (csrc/tn_bias_math.h), indices within
 * the molecule - and each point has its own final targets t_fin [G, D].  Every point is minimised with its CVs held at exact values
 * t_cur, which move from the CVs of the start geometry to t_fin by at most drive_d per step.  Per step, after the evaluation F(x),
 * per point, in fp64 on the widened fp32 positions (csrc/tn_scan_math.h):
 *   the CVs s_d and gradients g_d, rows on fixed atoms zero;  M = g g^T (D x D);  M lambda = g.F and M mu = g.v by Cholesky;
 *     lambda and mu are rounded to fp32 once
 *   F_perp = F - sum_d lambda_d g_d,  v_perp = v - sum_d mu_d g_d:  on a CV atom the correction is the fp64 sum in (CV, slot) order,
 *     rounded to fp32 once and added with one md_add; other atoms are untouched
 *   FIRE's sums vf, ff, vv, fmax2 of (v_perp, F_perp) over the atoms that are not fixed, in the minimiser's fixed order, and
 *     tn_min::fire_control, unchanged, one controller per point: a point converges when sqrt(fmax2) < fmax AND t_cur = t_fin; until
 *     the targets have arrived the controller is handed a bound of zero.  A converged point is frozen bit for bit
 *   the move tn_min::atom_move on (v_perp, F_perp)
 *   the drive  t_cur_d <- t_cur_d + clamp(diff(t_fin_d, t_cur_d), +-drive_d), exactly t_fin_d on arrival; a torsion goes the short way
 *   the constraint step on the fp64 positions of the CV atoms: up to max_iter corrections x <- x - sum_d nu_d g_d with
 *     (g g^T) nu = sigma, sigma_d = diff(s_d(x), t_cur_d), gradients at the current iterate, until max_d |sigma_d| < tol; then the
 *     CV atoms that are not fixed are rounded to fp32 once and written
 * At a constrained minimum dE/dt_d = -lambda_d: the logged multiplier is the mean force along the scan.
 * A point that still moves is unusable - status 2 - when a FIRE sum or its energy is not finite (cause 1), a CV or a gradient is not
 * finite (2), the Gram matrix has a pivot that is not positive and finite (3: two identical CVs, a CV whose atoms are all fixed) or
 * the constraint step did not converge in max_iter corrections (4).  Causes 1 to 3 are found before anything of the step is accepted.
 * The constraint step follows the move, so it writes nothing when it fails - neither positions nor the driven t_cur - and flags its point; the controller of the next step
 * latches cause 4 and the x and v the move had saved are put back.  Overflow is the minimiser's protocol (status 1, x and v put
 * back).  Only the single-block controller writes the status word; every later launch changes nothing until a reset. */
/* Bytes of the state `scan_ws`: the header, per point the controller's state, targets, CVs, multipliers, the corrections of the <= 16
 * CV atoms and the slice sums, and per atom the saved x and v (24 bytes).  n_atoms >= 1, n_points >= 1. */
int tmdnet_scan_workspace_bytes(int64_t n_atoms, int64_t n_points, size_t* bytes);
/* Step counter = step0, status cleared, every point moving again with dt0 > 0 and alpha0.  The first launch after it must be
 * tmdnet_scan_advance(TMDNET_MIN_CLOSE) on the start geometry: it sets t_cur to the CVs found there and counts no step. */
int tmdnet_scan_reset(void* stream, void* scan_ws, int64_t n_atoms, int64_t n_points, uint64_t step0, double dt0, double alpha0);
/* Enqueues one phase (TMDNET_MIN_OPEN / MIDDLE / CLOSE with the minimiser's meaning).  MIDDLE is four launches - the projection and
 * the sums on a grid (point, slice of <= 1 024 atoms), every block forming its point's multipliers itself with the same bits; the
 * controller as one block; one thread per atom; one wave per point for the drive and the constraint step - CLOSE the first three, OPEN
 * the last two: a replay of K steps is 4 K + 1 launches besides the evaluations.  Nothing allocates or synchronises.
 *   m, graph_ws   as for tmdnet_min_advance (both NULL: no overflow counter is looked at).
 *   pos, vel [n_points n, 3]   read and rewritten.
 *   forces        MIDDLE / CLOSE: the evaluation's F [n_points n, 3];  OPEN: projected_keep.
 *   energy        [n_points], required for MIDDLE / CLOSE.
 *   fixed [n] or NULL.
 *   forces_keep, projected_keep [n_points n, 3]   receive F and F_perp once the step is accepted; forces_keep may be NULL.
 *   n_cv, cv_kind [n_cv], cv_atoms [n_cv, 4]   HOST arrays, read during the call: kinds 0 distance, 1 angle, 2 torsion; unused
 *                 slots are ignored.  TMDNET_ERR_INVALID for n_cv outside 1..4, an index outside 0..n-1 or repeated within a CV.
 *   targets [n_points, n_cv] fp64, device.  drive [n_cv] fp64 > 0, HOST.  tol > 0, max_iter >= 1.
 *   the FIRE parameters and the seven log rows of tmdnet_min_advance, one entry per point.
 *   log rows      cv, target [n_points, n_cv] fp64 (s and t_cur at the evaluation); multiplier [n_points, 2, n_cv] fp32 (lambda, mu);
 *                 correction [n_points, A, 2, 3] fp32 (of F and v on the A distinct CV atoms, ascending); constrained
 *                 [n_points, A, 3] fp32 and iterations [n_points] int32 (the CV atoms after this launch's constraint step and its
 *                 number of corrections; MIDDLE and OPEN).  Each may be NULL. */
int tmdnet_scan_advance(tmdnet_model* m, void* stream, void* graph_ws, void* scan_ws, int64_t n_atoms, int64_t n_points, int32_t phase,
                        float* pos, float* vel, const float* forces, const float* energy, const uint8_t* fixed, float* forces_keep,
                        float* projected_keep, int32_t n_cv, const int32_t* cv_kind, const int32_t* cv_atoms, const double* targets,
                        const double* drive, double tol, int32_t max_iter, double dt_max, int32_t n_min, double f_inc, double f_dec,
                        double alpha0, double f_alpha, double max_step, double fmax, float* epot_log_row, float* fmax_log_row,
                        double* sums_log_row, float* coef_log_row, double* dt_log_row, double* alpha_log_row, int64_t* converged_log_row,
                        double* cv_log_row, double* target_log_row, float* multiplier_log_row, float* correction_log_row,
                        float* constrained_log_row, int32_t* iterations_log_row);
/* tmdnet_min_status, and host[2] = the cause when status is 2: 1 a sum, 2 a CV or gradient, 3 the Gram matrix, 4 the constraint step. */
int tmdnet_scan_status(void* stream, void* scan_ws, uint64_t host[3]);

/* ---- Hessians and normal-mode preparation assembled on the device (csrc/tn_vib.hip; additive exports, the ABI revision stays 10) ----
 * The molecules of a batch are independent, so R replicas of a batch of B molecules and N atoms, each carrying ONE coordinate of
 * every molecule, give R Hessian columns of every molecule from one evaluation of the replicated batch: analytically, hv = H v of
 * tmdnet_loss_param_grads with a unit seed, or as a central difference of the forces of two tmdnet_energy_forces calls on displaced
 * copies.  These entries seed / displace the replicated batch, gather the columns into per-molecule matrices, and turn those into
 * the mass-weighted, projected matrices whose eigenvalues are the squared angular frequencies (Wilson, Decius and Cross, Molecular
 * Vibrations, 1955, ch. 2).  Everything is device memory; nothing is read back.
 * Numbering: the atoms of a molecule are contiguous, `batch` [N] is non-decreasing.  free_idx [n_free] lists the atoms that are not
 * fixed, in the caller's order; fstart [B + 1] holds the molecules' offsets into it.  Molecule b has D_b = 3 (fstart[b+1] - fstart[b])
 * coordinates, coordinate i = component i % 3 of its free atom i / 3, and dim = D >= max_b D_b (a multiple of 3) is the padded size.
 * Replica r of a pass that starts at column col0 carries column k = col0 + r of every molecule with k < D_b; a molecule with fewer
 * columns is neither seeded nor displaced in that replica.  Row r N + a of a replicated buffer is atom a of replica r (its molecule
 * index in the evaluation is r B + b); z, batch, q and the boxes are replicated by the caller. */
#define TMDNET_VIB_SEED 0
#define TMDNET_VIB_PLUS 1
#define TMDNET_VIB_MINUS 2
#define TMDNET_VIB_ANALYTIC 0
#define TMDNET_VIB_CENTRAL 1
#define TMDNET_VIB_PROJECT_NONE 0
#define TMDNET_VIB_PROJECT_TRANS 1
#define TMDNET_VIB_PROJECT_TRANS_ROT 2
#define TMDNET_VIB_INFO 8
/* Bytes tmdnet_vib_finish needs beyond the caller's buffers: per molecule the projection basis U [6, dim], U^T A [6, dim] and
 * U^T A U [6, 6] in fp64.  tmdnet_vib_seed and tmdnet_vib_gather need none. */
int tmdnet_vib_workspace_bytes(int64_t n_mol, int64_t dim, size_t* bytes);
/* One thread per replicated atom; out [replicas n_atoms, 3].  TMDNET_VIB_SEED: the seed vector, zero except 1.0 at the component a
 * replica carries (pos and delta are not read).  TMDNET_VIB_PLUS / MINUS: the replicated positions with that one component moved by
 * +delta / -delta in ONE rounded fp32 addition (the rounding contract of the MD loop); every other entry keeps the caller's bits.
 * A replica whose column is beyond every molecule's D_b (the padding of the last pass) is all zero / undisplaced. */
int tmdnet_vib_seed(void* stream, int32_t mode, int64_t n_atoms, int64_t n_mol, int64_t replicas, int64_t col0, const float* pos,
                    const int64_t* batch, const int64_t* free_idx, const int64_t* fstart, float delta, float* out);
/* The columns col0 .. col0 + replicas - 1 of every molecule into the padded row-major fp32 H [n_mol, dim, dim], which the caller zeroes
 * once before the first pass:
 *   TMDNET_VIB_ANALYTIC   H[b][i, k] = hv[r N + atom(b, i / 3)][i % 3]         (hv_or_f_plus = hv of the pass; the other three NULL)
 *   TMDNET_VIB_CENTRAL    H[b][i, k] = - (F+ - F-) / den, den = x+ - x- of the moved coordinate read from the two displaced position
 *                         buffers (the actual difference of the rounded positions, NOT 2 delta); difference and quotient in fp64,
 *                         rounded to fp32 once.  hv_or_f_plus / f_minus = the forces at pos_plus / pos_minus.
 * One thread per (replica, free coordinate).  Every (b, i, k) with i, k < D_b is written exactly once over the passes col0 = 0, R,
 * 2 R, ...; nothing outside those entries is written; no atomics.  replicas <= 65535. */
int tmdnet_vib_gather(void* stream, int32_t mode, int64_t n_atoms, int64_t n_mol, int64_t n_free, int64_t dim, int64_t replicas,
                      int64_t col0, const int64_t* batch, const int64_t* free_idx, const int64_t* fstart, const float* hv_or_f_plus,
                      const float* f_minus, const float* pos_plus, const float* pos_minus, float* H);
/* One block per molecule, fp64 throughout, every entry computed by one thread in a fixed order, no floating-point atomics: repeats
 * are bit-identical.  Writes A [n_mol, dim, dim] (fp64, zero in its padding) and info [n_mol, TMDNET_VIB_INFO] (fp64):
 *   info[0] hmax = max |H_ij|;  info[1] asym = max |H_ij - H_ji|;  info[2] drift = max_{i, beta} | sum_j H[i, 3 j + beta] |, the
 *     acoustic sum (meaningful only when no atom of the molecule is fixed);  info[3] the rank of the projection;  info[4] its mode;
 *     info[5] D_b;  info[6..7] zero
 *   S = (H + H^T) / 2;   A_ij = S_ij / sqrt(m_i m_j), masses [n_atoms] fp32 widened
 *   projection, per molecule: mode 0 (none) when mol_atoms [n_mol] (the molecules' atom counts, or NULL: no atom is fixed) says an
 *     atom of the molecule is fixed, else `project`: TMDNET_VIB_PROJECT_NONE, _TRANS (translations: a periodic system) or _TRANS_ROT.
 *     Candidates in mass-weighted coordinates, t_alpha[3 j + beta] = sqrt(m_j) delta_alpha,beta and r_alpha[3 j ..] = sqrt(m_j) (e_alpha x
 *     (x_j - c)), c the centre of mass from the fp32 positions widened, orthonormalised in the order t_x t_y t_z r_x r_y r_z by
 *     modified Gram-Schmidt applied twice; a candidate is kept when |w|^2 > 1e-12 |w0|^2 (rank 6 in general, 5 for a linear
 *     molecule, 3 for one atom).  With U the kept vectors:  A <- A - U (U^T A) - (U^T A)^T U^T + U (U^T A U) U^T.
 * info[3] = -1 and nothing else written: fstart does not fit dim. */
int tmdnet_vib_finish(void* stream, void* vib_ws, size_t ws_bytes, int64_t n_atoms, int64_t n_mol, int64_t dim, int32_t project,
                      const float* H, const float* pos, const float* masses, const int64_t* free_idx, const int64_t* fstart,
                      const int64_t* mol_atoms, double* A, double* info);

/* ---- pair priors: ZBL and D2 (csrc/tn_prior.hip, csrc/tn_prior_math.h) -------------------------------------------------------------
 * Parameter-free pair potentials of pos, z, batch and box that the reference adds to y after the head (models/model.py:612-615,
 * priors/zbl.py, priors/d2.py).  Here they are one separate pass BEHIND tmdnet_energy_forces / tmdnet_energy_forces_virial: it adds
 * its energies, forces and virial to what the model's pass wrote.  Brute force inside every molecule, three launches on the caller's
 * stream, no read-back, no synchronisation (capturable); no floating-point atomics, fixed summation order, bit-identical repeats.
 *   ZBL   u = (2.30707755e-28 / energy_scale / distance_scale) phi(r distance_scale / a) C(r) Z_i Z_j / r for 0 < r < cutoff, C the
 *         cosine cutoff, a = 0.8854 a_0 / (Z_i^0.23 + Z_j^0.23); r after the minimum image of the neighbour search when a box is given
 *   D2    u = - sqrt(C6_i C6_j) / R^6 / (1 + e^{-20 (R / (Rr_i + Rr_j) - 1)}) / (energy_scale N_A), R = r distance_scale 1e9, for
 *         0 < r < cutoff (a hard cutoff: no force term from it); never sees the box
 * The tables are indexed by the species z[i] (the prior's atomic_number map is already applied by the caller), fp32, on the host. */
#define TMDNET_PRIOR_ZBL 1
#define TMDNET_PRIOR_D2 2
#define TMDNET_PRIOR_MAX_MOLECULE_ATOMS 32768
typedef struct {
  int32_t flags;  /* TMDNET_PRIOR_ZBL | TMDNET_PRIOR_D2 */
  int32_t max_z;  /* length of every table; a species outside [0, max_z) yields NaN */
  double zbl_cutoff, zbl_distance_scale, zbl_energy_scale; /* cutoff in the caller's length unit; scales to metres and Joules */
  double d2_cutoff, d2_distance_scale, d2_energy_scale;
  const float* zbl_z;      /* [max_z] atomic number Z of species s (host) */
  const float* zbl_z23;    /* [max_z] Z^0.23 */
  const float* d2_sqrt_c6; /* [max_z] sqrt(C6) in sqrt(J/mol nm^6) */
  const float* d2_rr;      /* [max_z] van der Waals radius in nm */
} tmdnet_pair_priors;
/* Copies the tables to the device (synchronous) and derives the unit constants in fp64.  NULL or flags == 0 clears the priors. */
int tmdnet_set_pair_priors(tmdnet_model* m, const tmdnet_pair_priors* priors);
/* Workspace of one pass: two int32 range counters per molecule and one row of 8 doubles per atom.  The caller ZEROES it before the first
 * pass and again whenever n_atoms or n_mol differ from the previous pass on it; every pass leaves the counters at zero. */
int tmdnet_pair_priors_workspace_bytes(const tmdnet_model* m, int64_t n_atoms, int64_t n_mol, size_t* bytes);
/* ADDS the priors to energy [n_mol], forces [n_atoms, 3] (NULL: energies only) and virial [n_mol, 9] (NULL: none; the convention of
 * tmdnet_energy_forces_virial).  pos, z, batch, box (box_mode 0: none, 1: one [3,3] box, 2: one per molecule) as given to
 * tmdnet_build_graph, in the caller's atom order; the batch need not be sorted.  TMDNET_ERR_INVALID when atom_weights is not NULL or
 * atom weights / a halo exchange are set on the handle (domain decomposition has no prior path), or when n_atoms exceeds
 * TMDNET_PRIOR_MAX_MOLECULE_ATOMS per molecule on average (the caller checks the individual molecules);  TMDNET_ERR_STATE without
 * priors set. */
int tmdnet_pair_priors_add(tmdnet_model* m, void* stream, void* ws, size_t ws_bytes, int64_t n_atoms, int64_t n_mol, const float* pos,
                           const int64_t* z, const int64_t* batch, const float* box, int32_t box_mode, const float* atom_weights,
                           float* energy, float* forces, float* virial);
/* Test entry: the same pass into ZEROED outputs (it zeroes them and the workspace's counters itself), plus the per-atom energies
 * e_i = 1/2 sum_j u_ij as fp64 [n_atoms] (NULL: not returned).  forces and virial may be NULL. */
int tmdnet_debug_prior(tmdnet_model* m, void* stream, void* ws, size_t ws_bytes, int64_t n_atoms, int64_t n_mol, const float* pos,
                       const int64_t* z, const int64_t* batch, const float* box, int32_t box_mode, float* energy, float* forces,
                       float* virial, double* e_atom);

/* ---- committee of models (csrc/tn_committee.hip, csrc/tn_committee_math.h; additive exports, the ABI revision stays 10) -----------
 * M members, 2 <= M <= TMDNET_COMMITTEE_MAX_MEMBERS, have each written their energies E_k [n_mol] and forces F_k [n_atoms, 3] (fp32,
 * the caller's atom order) - by tmdnet_energy_forces on the same stream, or by anything else.  One pass reduces them:
 *   mean_m = (1 / M) sum_k E_k,m        std_m = sqrt(sum_k (E_k,m - mean_m)^2 / (M - 1))    (unbiased: torch.std)
 *   the same per force component;  d_i = sqrt(sum_c std_i,c^2), a d_i that is not finite is +inf;
 *   D_m = max_{i in m} d_i and a_m the smallest atom index that attains it; a molecule without atoms has D_m = 0, a_m = -1.
 * Two passes over the M values (the mean, then the squared differences), sums, division and square roots in fp64 in member order,
 * every output rounded to fp32 once.  Two launches, no read-back, nothing allocated, capturable; the molecule maximum is a 64-bit
 * integer atomicMax, so repeats are bit-identical and `batch` need not be sorted (entries outside [0, n_mol) join no molecule).
 * The gate compares as !(D_m <= threshold): a NaN never passes as certain. */
#define TMDNET_COMMITTEE_MAX_MEMBERS 16
#define TMDNET_COMMITTEE_FLAG 1 /* record the first step at which !(D_m <= flag_above), per molecule; the trajectory goes on */
#define TMDNET_COMMITTEE_STOP 2 /* latch status 6 in md_ws after the step at which any molecule has !(D_m <= stop_above) */
typedef struct {
  int32_t flags;           /* TMDNET_COMMITTEE_FLAG | TMDNET_COMMITTEE_STOP; 0: no gate, md_ws only freezes the pass with the loop */
  float flag_above;        /* thresholds on D_m, in the unit of the forces; not NaN */
  float stop_above;
  void* md_ws;             /* the loop's tmdnet_md_workspace_bytes state: status word and step counter; required with flags != 0 */
  int64_t* flagged_at;     /* [n_mol], -1 before: the step (1 = the first after tmdnet_md_reset(0)) molecule m was first flagged at */
  float* flagged_dev;      /* [n_mol] D_m of that step */
  int64_t* flagged_atom;   /* [n_mol] a_m of that step */
  float* flagged_pos;      /* [n_atoms, 3]: the molecule's atoms at that step; rows of unflagged molecules are not written */
} tmdnet_committee_gate;
/* Workspace of the pass: a 256-byte header (the stop word and the record of a stop), one 64-bit word and one int32 per molecule.
 * The caller ZEROES it once (or calls tmdnet_committee_reset); every pass leaves the per-molecule words at zero. */
int tmdnet_committee_workspace_bytes(int64_t n_atoms, int64_t n_mol, size_t* bytes);
/* Enqueues a memset of the whole workspace: words, decisions and the record of a stop. */
int tmdnet_committee_reset(void* stream, void* ws, int64_t n_mol);
/* The pass.  energies / forces_in: HOST arrays of n_members device pointers, read during the call and passed to the kernels by value
 * (no pointer table in device memory).  Outputs: energy, energy_std, max_deviation [n_mol], max_atom [n_mol] int64, forces,
 * forces_std [n_atoms, 3], deviation [n_atoms].
 *   members, graph_ws   both NULL, or HOST arrays of the n_members handles and the graph workspaces of the evaluations before this
 *                 call (static shapes): the overflow flags of members 1.. are folded into member 0's, which is the flag the
 *                 integrator reads when it is given member 0's handle and workspace; an overflowed evaluation logs and decides nothing.
 *   gate          NULL, or the gate of a captured MD step: with its md_ws a frozen loop (status != 0) leaves every output alone;
 *                 with TMDNET_COMMITTEE_FLAG the molecule's thread records flagged_at / flagged_dev / flagged_atom, with
 *                 TMDNET_COMMITTEE_STOP it enters the stop word.  The step is md_ws's counter + 1: call this BEFORE the closing launch.
 * TMDNET_ERR_INVALID before any launch: n_members outside 2..16, a NULL array or entry, negative or oversized counts, only one of
 * members / graph_ws, unknown gate flags, gate flags without md_ws, TMDNET_COMMITTEE_FLAG without its four buffers, a NaN threshold.
 * TMDNET_ERR_WORKSPACE: ws_bytes too small. */
int tmdnet_committee_reduce(void* stream, void* ws, size_t ws_bytes, int32_t n_members, const float* const* energies,
                            const float* const* forces_in, int64_t n_atoms, int64_t n_mol, const int64_t* batch, float* energy,
                            float* forces, float* energy_std, float* forces_std, float* deviation, float* max_deviation,
                            int64_t* max_atom, tmdnet_model* const* members, void* const* graph_ws, const tmdnet_committee_gate* gate);
/* The gate's second half, one launch AFTER the closing launch of the step (tmdnet_md_advance TMDNET_MD_CLOSE with the committee's
 * forces and energy; it does not move positions): copies the atoms of the molecules flagged at this step from pos into
 * gate->flagged_pos, and turns a stop word into status 6 of gate->md_ws - from there every launch of the loop returns at once, as
 * after an overflow - and the record {step, molecule, atom, D}: the molecule of the largest D_m (the smallest index among equals)
 * and max_atom[molecule], the row the pass wrote for this step.  The frozen state is the completed step: pos, vel and forces_keep of
 * that step, the counter at that step.  tmdnet_md_status answers TMDNET_ERR_STATE with host[1] = 6.  gate->flags == 0: no launch.
 * A step is then: M evaluations, tmdnet_committee_reduce, TMDNET_MD_CLOSE, tmdnet_committee_latch, and TMDNET_MD_OPEN on
 * forces_keep when another step follows - TMDNET_MD_MIDDLE is CLOSE then OPEN on the same values, so the split changes no bit. */
int tmdnet_committee_latch(void* stream, void* ws, int64_t n_atoms, int64_t n_mol, const int64_t* batch, const float* pos,
                           const int64_t* max_atom, const tmdnet_committee_gate* gate);
/* host[0] = 1 when a stop was latched since the last reset, then host[1] = step, host[2] = molecule, host[3] = atom, host[4] = the
 * bits of D (fp32) in the low word.  Synchronises the stream. */
int tmdnet_committee_status(void* stream, void* ws, uint64_t host[5]);

/* ---- Minima hopping: a conformer search inside a captured step (csrc/tn_hop.hip; additive exports, the ABI revision stays 10) ----
 * Goedecker, J. Chem. Phys. 120, 9911 (2004); parameters named as in ASE's MinimaHopping.  The n_mol molecules of the batch are
 * independent walkers.  A step is ONE evaluation (E, F at pos) and tmdnet_hop_advance; every walker is in one phase for the whole
 * step, and walkers in different phases share the evaluation (csrc/tn_hop_math.h holds every statement below):
 *   QUENCH   FIRE as in tmdnet_min_advance (unit masses, ASE's clamp), one controller per walker.  sqrt(max |f|^2) < fmax: the
 *            walker does not move and goes to COMPARE.  After opt_steps moves without that (never for the quench of the start
 *            geometry): outcome UNCONVERGED, the walker is put back on its current minimum, kT and ediff stay, new velocities are
 *            drawn, LAUNCH follows.
 *   COMPARE  one step; its evaluation repeats the last one.  For the current minimum and every live ring entry whose energy lies
 *            within energy_tol of E, 18 fp64 sums of the pair (fresh geometry a, reference b) - n, sum a, sum b, sum a.a, sum b.b,
 *            sum a_i b_j - give rmsd^2: align 2 (rotation) Horn's quaternion method, the largest eigenvalue of the 4 x 4 matrix of
 *            the centred cross-covariance by 12 cyclic Jacobi sweeps, proper rotations only; align 1 (translation, and molecules of
 *            fewer than 3 atoms) the centred sum; align 0 the plain sum.  In this order: no current minimum yet - START: recorded
 *            (unless a kept history holds it), accepted, no parameter changes; the current minimum again (rmsd < rmsd_tol and
 *            |dE| < energy_tol) - SAME, kT *= beta1; a ring entry - KNOWN, kT *= beta2, its visits + 1; otherwise NEW, kT *= beta3,
 *            written to ring slot n_recorded mod capacity (the oldest entry is overwritten; n_recorded counts the START too) and
 *            to `best` when it is the lowest ever, then ACCEPTED when E < E_cur + ediff (ediff *= alpha1; it becomes the current
 *            minimum) or REJECTED (ediff *= alpha2).  Every outcome but START counts one hop.  The per-atom kernel copies pos into
 *            the current minimum or puts the current minimum back into pos, then draws v = (sqrt(kT) sig_i) xi with xi from
 *            normals3 on Philox4x32-10, key = seed, counter = (hop count lo, hi, the caller's atom index, 2).  LAUNCH follows.
 *   LAUNCH   sums about the centroid of the current minimum: sum m, m d, m v, m d x v and the six second moments - and f.f, only so
 *            that forces that are not finite are found before the launch's opening half-step consumes them.  v_com, and with
 *            align 2 omega = I^-1 L about the centre of mass by an fp64 LDL^T solve (a pivot below 1e-10 of the trace: omega = 0 and
 *            outcome SINGULAR); v <- v - (u + omega x d), u = v_com - omega x d_cm, then the opening half of an MD step.  E_0 = E.
 *   MD       NVE: the closing and the opening half of tmdnet_md_advance's fused step.  E_k is appended; a minimum of the energy
 *            along the escape is counted at k >= 2 when E_{k-1} < E_{k-2} and E_{k-1} <= E_k.  With mdmin minima counted, or at
 *            k = md_steps, the escape ends in this step: v = 0, FIRE starts afresh (dt0, alpha0) and moves at once from
 *            (v.f = 0, f.f, v.v = 0, max |f|^2); QUENCH follows.
 * Fixed atoms (fixed[i] != 0; hk = sig = 0) never move, have zero velocity and enter no sum but those of COMPARE.
 * Rounding: what moves an atom is fp32, one rounding per operation in the order written; the sums of LAUNCH and COMPARE are fp64
 * products of widened fp32 values; everything per walker is fp64 and rounded to fp32 once where atoms consume it.  Sums are reduced
 * in a fixed order without floating-point atomics: repeats are bit-identical.
 * Status: 1 an evaluation overflowed the neighbour list (x and v of the last move are put back), 2 an energy or a sum of a walker
 * was not finite (nothing of that step is written).  Either freezes everything until tmdnet_hop_reset. */
#define TMDNET_HOP_QUENCH 0
#define TMDNET_HOP_COMPARE 1
#define TMDNET_HOP_LAUNCH 2
#define TMDNET_HOP_MD 3
#define TMDNET_HOP_ALIGN_NONE 0
#define TMDNET_HOP_ALIGN_TRANSLATION 1
#define TMDNET_HOP_ALIGN_ROTATION 2
/* Parameters and buffers of a hop step.  Everything behind a pointer is device memory and stays the caller's; N = n_atoms,
 * B = n_mol, C = capacity. */
typedef struct tmdnet_hop_args {
  double dt_max, f_inc, f_dec, alpha0, f_alpha, max_step, fmax, dt0; /* FIRE, as tmdnet_min_advance / tmdnet_min_reset */
  double beta1, beta2, beta3, alpha1, alpha2;                        /* the feedback on kT and ediff */
  double rmsd_tol, energy_tol;                                       /* > 0 */
  uint64_t seed;
  float dt;                                                          /* the MD time step */
  int32_t n_min;                                                     /* FIRE */
  int32_t mdmin, md_steps, opt_steps;                                /* >= 1 */
  int32_t capacity;                                                  /* 1..64 ring entries per walker */
  int32_t align;                                                     /* TMDNET_HOP_ALIGN_* */
  float* pos;              /* [N, 3] read and rewritten */
  float* vel;              /* [N, 3] read and rewritten: the MD velocity or FIRE's */
  const float* forces;     /* [N, 3] of this step's evaluation */
  const float* energy;     /* [B] */
  const float* hk;         /* [N] dt force_scale / (2 m); 0 for a fixed atom */
  const float* mass;       /* [N] */
  const float* sig;        /* [N] sqrt(force_scale / m); 0 for a fixed atom */
  const uint8_t* fixed;    /* [N] or NULL */
  const int64_t* batch;    /* [N]; may be NULL for one molecule */
  float* forces_keep;      /* [N, 3] or NULL: receives F of every accepted step */
  float* cur_pos;          /* [N, 3] the minimum every walker hops from */
  float* best_pos;         /* [N, 3] the lowest minimum ever recorded */
  float* ring_pos;         /* [C, N, 3] */
  double* ring_energy;     /* [B, C] */
  int64_t* ring_found;     /* [B, C] the step an entry was recorded at */
  int64_t* ring_visits;    /* [B, C] */
  double* kT;              /* [B] the walkers' public state, rewritten by every step */
  double* ediff;           /* [B] */
  double* cur_energy;      /* [B] */
  double* best_energy;     /* [B] */
  int32_t* phase;          /* [B] the phase of the NEXT step */
  int64_t* counters;       /* [B, 7] n_hops, n_same, n_known, n_new, n_accepted, n_unconverged, n_recorded */
  float* epot_row;         /* log rows of this step, each [B] unless noted, each may be NULL */
  float* fmax_row;         /* QUENCH and MD steps; 0 otherwise */
  float* ekin_row;         /* MD steps: sum 0.5 m v^2 of the closed velocities, in the unit of m v^2; 0 otherwise */
  int32_t* phase_row;      /* the phase the step ran in */
  int32_t* outcome_row;    /* 0 none, 1 START, 2 SAME, 3 KNOWN, 4 ACCEPTED, 5 REJECTED, 6 UNCONVERGED, 7 SINGULAR */
  double* sums_row;        /* [B, 16]: the phase's sums (QUENCH v.f, f.f, v.v, max |f|^2; MD ekin, f.f, 0, max |f|^2; LAUNCH its first 16;
                              COMPARE rmsd^2 to the current minimum or -1, the smallest rmsd^2 to a ring entry looked at or -1, n) */
  float* coef_row;         /* [B, 10]: c_v, c_f, d of FIRE, u and omega of a launch, sqrt(kT) of a draw */
} tmdnet_hop_args;
/* Bytes of the state `hop_ws`: the header, per walker its state, its decision and 18 (capacity + 1) sums (times the slices of a
 * molecule of more than 1 024 atoms), per atom the saved x and v.  n_atoms >= 1, n_mol >= 1, capacity 1..64. */
int tmdnet_hop_workspace_bytes(int64_t n_atoms, int64_t n_mol, int32_t capacity, size_t* bytes);
/* Step counter = step0, status cleared, every walker in QUENCH of the geometry at args->pos with kT0[b], ediff0[b] (device, [B] fp64),
 * FIRE at its start values and no current minimum; args->vel must be zero.  keep_history == 0: counters zero and the ring empty;
 * otherwise ring, best and counters stay.  Rewrites the public state (kT, ediff, cur_energy, best_energy, phase, counters); of args it
 * reads only the parameters, pos and vel: every other pointer may be NULL here. */
int tmdnet_hop_reset(void* stream, void* hop_ws, int64_t n_atoms, int64_t n_mol, const tmdnet_hop_args* args, uint64_t step0,
                     const double* kT0, const double* ediff0, int32_t keep_history);
/* Enqueues the launches of one step after its evaluation: the reduction on a grid (walker, slice of <= 1 024 atoms), its finish
 * pass when a molecule has more than one slice, the controller as one block, one thread per atom.  Nothing allocates or
 * synchronises; `args` is read during the call.
 *   m, graph_ws   the handle and graph workspace of the evaluation (the overflow counter and the molecules' atom ranges), or both
 *                 NULL: then no overflow counter is looked at and a walker's atoms are those with batch[i] = b, so any forces and
 *                 energies can be fed.
 * TMDNET_ERR_INVALID before any launch for a NULL buffer other than fixed / batch (one molecule) / forces_keep / the log rows, a
 * parameter outside its range, or a shape tmdnet_hop_workspace_bytes refuses. */
int tmdnet_hop_advance(tmdnet_model* m, void* stream, void* graph_ws, void* hop_ws, int64_t n_atoms, int64_t n_mol,
                       const tmdnet_hop_args* args);
/* host[0] = the step counter, host[1] = the status.  TMDNET_ERR_OVERFLOW for status 1, TMDNET_ERR_STATE for 2.  Synchronises. */
int tmdnet_hop_status(void* stream, void* hop_ws, uint64_t host[2]);

#ifdef __cplusplus
}
#endif
#endif /* TMDNET_AMD_H */
