"""ctypes binding of libxeq_hip.so (the C ABI declared in include/xeq.h).

There is NO CPU fallback: if the HIP library is missing the import of any op
raises, and every op rejects non-HIP tensors.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_int, c_int32, c_int64, c_uint64, c_void_p
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("XEQ_LIB_PATH") or os.path.join(_HERE, "libxeq_hip.so")   # XEQ_LIB_PATH: development builds

XEQ_F32, XEQ_F64 = 0, 1
COPY_MANY_MAX = 16       # XEQ_COPY_MANY_MAX of include/xeq.h
# (tests/test_resident_records_host.py holds the next five lines against the header)
MD_CHUNK = 256          # XEQ_MD_CHUNK of include/xeq.h: atoms per kinetic-energy chunk (md.py, optimize.py)
MD_NVE, MD_LANGEVIN, MD_BERENDSEN, MD_PURPOSE_LANGEVIN, MD_PURPOSE_MAXWELL = 0, 1, 2, 0, 1      # XEQ_MD_* of include/xeq.h (md.py)
NPT_BOX, NPT_CELL, NPT_INV, NPT_CELL_NEXT, NPT_INV_NEXT, NPT_MU, NPT_P, NPT_V = 40, 0, 9, 18, 27, 36, 37, 38      # XEQ_NPT_* of include/xeq.h (md.py)
FIRE_FRESH, FIRE_ACTIVE, FIRE_CONVERGED = 0, 1, 2      # XEQ_FIRE_* of include/xeq.h
# XEQ_NVT_* of include/xeq.h (md.py's canonical thermostats; tests/test_nvt_host.py holds these two lines against the header)
NVT_ROW, NVT_MAX_CHAIN, NVT_GAMMA_TRIES, NVT_PURPOSE, NVT_SCALE, NVT_BATH, NVT_XI, NVT_VXI = 18, 8, 16, 2, 0, 1, 2, 10
NVT_NOSE_HOOVER, NVT_BUSSI, REC_NVT = 0, 1, 16          # (REC_NVT: XEQ_REC_NVT, the record's number for xeq_record_bytes)
LBFGS_FRESH, LBFGS_ACTIVE, LBFGS_CONVERGED, LBFGS_MAX_MEMORY = 0, 1, 2, 32      # XEQ_LBFGS_* of include/xeq.h (optimize.LBFGS)
VIB_MAX_DIM, VIB_MAX_SWEEPS = 96, 30     # XEQ_VIB_MAX_DIM, XEQ_VIB_MAX_SWEEPS of include/xeq.h (vibrations.py)
VIB_LARGE_MAX_DIM = 768              # XEQ_VIB_LARGE_MAX_DIM: the cap of xeq_vib_eigh_large
VIB_ROTORS = ("atom", "linear", "nonlinear")      # XEQ_VIB_ATOM, _LINEAR, _NONLINEAR
SB_ACCUM_VEC = 16        # XEQ_SB_ACCUM_VEC of include/xeq.h: xeq_message_bwd_sb adds dL/dvec to the buffer it is handed
XHAT_HIGHER_L_ZERO = 2   # XEQ_XHAT_HIGHER_L_ZERO of include/xeq.h: hint bit on the xhat_layout argument of the wq message kernels
SB_Y0_ZERO = 8           # XEQ_SB_Y0_ZERO / XEQ_SB_Q_ACCUMULATE: the training-pass forms of the sb message kernels (ops.DiffMessage)
SB_Q_ACCUMULATE = 16
SB_NO_GY = 32
WQ_MIRROR_WALK = 4       # XEQ_WQ_MIRROR_WALK: the reverse wq kernel walks the forward plan of a symmetric list
WQ_PACKED_WEIGHTS = 64   # XEQ_WQ_PACKED_WEIGHTS: w_rbf of the wq message kernels is the packed copy (xeq_message_wq_pack_weights)
WQ_MAX_PART_SETS = 8     # XEQ_WQ_MAX_PART_SETS: sets of per-block partials one xeq_message_wq_edge_grad_sum launch adds up
RBF_KINDS = {"bessel": 0, "gaussian": 1, "expbern": 2, "expnorm": 3}
CUTOFF_KINDS = {"cosine": 0, "polynomial": 1}

_P = c_void_p
_I3 = ctypes.POINTER(c_int32)


def _record(c_name: str, *groups):
    """The ctypes.Structure of one argument record of include/xeq.h: ``groups`` = (type, "member names") in the header's order."""
    return type(c_name, (ctypes.Structure,), {"_fields_": [(name, kind) for kind, names in groups for name in names.split()]})


# The argument records of the resident drivers' front / back entries (resident.py) and of the neighbour search, member for member those
# of include/xeq.h; every member is 8 bytes wide.  In the order of XEQ_REC_*: load() holds their sizes against xeq_record_bytes.
ResSystem = _record("xeq_res_system", (c_int64, "dtype n n_graphs n_chunks"), (_P, "pos vel frc image batch book cell pbc"))
ResStep = _record("xeq_res_step", (_P, "frc_step energy_step n_edges_step virial_step reps_needed"), (c_int64 * 3, "reps"))
ResChunks = _record("xeq_res_chunks", (_P, "chunk_atom0 chunk_n graph_chunk_ptr partial partial_bad"))
ResRecorder = _record("xeq_res_recorder", (c_int64, "every start rows"), (_P, "traj_pos traj_epot traj_second traj_step traj_cell traj_pressure"))
MdParams = _record("xeq_md_params", (c_int64, "ensemble"), (_P, "inv_mass half_mass ke epot tfac rng_id"), (c_uint64, "seed"),
                   (c_double, "c1 noise2 dt_over_tau t0 half_dt"))
NptParams = _record("xeq_npt_params", (_P, "box step_cell virial reps_seen"), (c_double, "kappa p0 p_unit"))
FireParams = _record("xeq_fire_params", (_P, "fixed epot fmax dt alpha n_pos status converged_at coef"), (c_double, "fmax_tol maxstep dtmax"),
                     (c_int64, "n_min"), (c_double, "f_inc f_dec alpha_start f_alpha"))
# The neighbour search's record (ops._neighbor_list); kinds: XEQ_NEIGHBORS_* of include/xeq.h
NeighborSearch = _record("xeq_neighbor_search", (c_int64, "dtype kind n_graphs n_nodes n_cells"), (c_double, "cutoff"), (c_int64 * 3, "reps"),
                         (_P, "pos ptr img cells shift recip thr lo inv_w nbins bin_base bin_start bin_atom"))
NEIGHBORS_OPEN_SWEEP, NEIGHBORS_OPEN_BINS, NEIGHBORS_PBC_ALL, NEIGHBORS_PBC_PRUNED, NEIGHBORS_PBC_BINS = range(5)
LbfgsParams = _record("xeq_lbfgs_params", (_P, "fixed hist_s hist_y pending_s gram delta count head status dropped converged_at epot fmax ticket"),
                      (c_int64, "memory max_graph_chunks"), (c_double, "fmax_tol alpha maxstep damping"))
# The thermostats' record: its number stands apart from the dense run of RECORDS (include/xeq.h: XEQ_REC_NVT)
NvtParams = _record("xeq_nvt_params", (c_int64, "kind"), (_P, "state n_free graph_rng_id"), (c_int64, "chain_length"), (c_double, "kT tau dt"))
RECORDS_APART = {REC_NVT: NvtParams}
RECORDS = [ResSystem, ResStep, ResChunks, ResRecorder, MdParams, NptParams, FireParams, NeighborSearch, LbfgsParams]
_R = ctypes.POINTER


def fill(record, **members):
    """Set the named members of an argument record and return it.  A tensor gives its address, a ctypes array (host data) its own, None
    is NULL; the caller keeps both alive.  A name the record does not have is an error, not a new Python attribute."""
    kinds = dict(record._fields_)
    for name, value in members.items():
        if name not in kinds:
            raise AttributeError(f"{type(record).__name__} has no member {name!r}")
        if isinstance(value, torch.Tensor):
            value = value.data_ptr()
        elif isinstance(value, ctypes.Array) and kinds[name] is _P:
            value = ctypes.addressof(value)
        setattr(record, name, value)
    return record


# name -> argtypes, exactly the prototypes of include/xeq.h
_PROTOS = {
    "xeq_launch_count": [],
    "xeq_launch_names": [c_int64, c_char_p, c_int64],
    "xeq_csr_rowptr": [_P, c_int64, c_int64, _P, _P],
    "xeq_csr_by_key_workspace": [c_int64, c_int64],
    "xeq_csr_by_key": [_P, c_int64, c_int64, _P, c_int64, _P, _P, _P],
    "xeq_csr_by_key_bounded": [_P, c_int64, c_int64, _P, _P, c_int64, _P, _P, _P],
    "xeq_exclusive_scan_i32": [_P, c_int64, _P, _P],
    "xeq_exclusive_scan_i32_workspace": [c_int64],
    "xeq_exclusive_scan_i32_ws": [_P, c_int64, _P, _P, c_int64, _P],
    "xeq_reverse_edge_map": [_P, c_int64, c_int64, _P, _P, _P],
    "xeq_reverse_edge_map_pbc": [c_int, _P, _P, c_int64, c_int64, _P, _P, _P],
    "xeq_neighbors_bin_ids": [_R(NeighborSearch), _P, _P],
    "xeq_neighbors_count": [_R(NeighborSearch), _P, _P],
    "xeq_neighbors_fill": [_R(NeighborSearch), _P, c_int64, _P, _P, _P, _P],
    "xeq_pbc_image_counts": [c_int, _P, c_int64, _I3, c_double, _I3],
    "xeq_pbc_tables_host": [c_int, _P, c_int64, _I3, c_double, _P, c_int64],
    "xeq_pbc_wrap": [c_int, _P, _P, c_int64, c_int64, _P, _P, _I3, _P, _P, _P],
    "xeq_edge_vectors_fwd": [c_int, _P, _P, c_int64, _P, _P, _P, _P, _P, _P],
    "xeq_edge_vectors_bwd": [c_int, _P, c_int64, _P, _P, _P, _P, _P, _P],
    "xeq_sph_harm_fwd": [c_int, _P, c_int64, _I3, c_int, _P, _P],
    "xeq_sph_harm_bwd": [c_int, _P, _P, c_int64, _I3, c_int, _P, _P],
    "xeq_radial_fwd": [c_int, _P, c_int64, c_int, c_int, c_int, c_double, _P, _P, _P, _P, _P],
    "xeq_elementwise_tp_fwd": [c_int, _P, _P, c_int64, c_int64, _I3, _P, _P],
    "xeq_channel_dot_fwd": [c_int, _P, _P, c_int64, _I3, _P, _P],
    "xeq_eqln_fwd": [c_int, _P, _P, _P, c_int64, _I3, c_double, _P, _P],
    "xeq_eqln_bwd": [c_int, _P, _P, _P, c_int64, _I3, c_double, _P, _P],
    "xeq_segment_sum": [c_int, _P, _P, c_int64, c_int64, _P, _P],
    "xeq_linear_supported": [c_int, c_int, c_int],
    "xeq_mfma_order_probe": [_P, _P, _P, _P],
    "xeq_linear_fwd": [_P, c_int64, c_int64, c_int, _P, _P, c_int, c_int, c_int, _P, _P, c_int64, _P],
    "xeq_head_dot": [_P, c_int64, c_int, _P, _P, _P, _P],
    "xeq_head_bwd_hidden": [_P, c_int64, c_int, _P, _P, _P, _P],
    "xeq_head_supported": [c_int, c_int, c_int],
    "xeq_head_fwd": [_P, c_int64, c_int64, c_int, c_int, _P, _P, _P, _P, _P, _P, _P],
    "xeq_head_bwd": [_P, c_int64, c_int, _P, c_int64, _P, c_int64, _P, _P, _P],
    "xeq_electronic_supported": [c_int, c_int],
    "xeq_electronic_fwd": [c_int, _P, c_int64, c_int64, c_int, _P, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "xeq_first_block_front": [_P, c_int, c_int64, c_int64, _P, _P, _P, c_int, c_int, c_int64, _P, _P, _P, _P],
    "xeq_rowptr_from_degrees": [_P, c_int64, c_int64, _P, _P, _P, _P],
    "xeq_rowptr_from_degrees_max": [],
    "xeq_wgrad_chunks": [c_int64, c_int, c_int],
    "xeq_wgrad": [_P, c_int64, _P, c_int64, c_int64, c_int, c_int, c_int, c_int, _P, _P],
    "xeq_load_padded_batch": [c_int, _P, _P, _P, _P, c_int64, c_int64, c_int64, c_int64, c_double, c_double, _P, _P, _P, _P, _P],
    "xeq_load_padded_batch_z64": [c_int, _P, _P, _P, _P, c_int64, c_int64, c_int64, c_int64, c_double, c_double, _P, _P, _P, _P, _P],
    "xeq_load_padded_shard": [c_int, _P, _P, c_int, _P, _P, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_double, c_double, _P, _P, _P, _P, _P],
    "xeq_copy_many": [c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64), _P],
    "xeq_compare_many": [c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), ctypes.POINTER(c_int64), ctypes.c_int32, _P, _P],
    "xeq_tensor_product_path": [c_int, _P, _P, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                c_int, c_int, _P, _P, c_int64, c_double, _P, _P],
    "xeq_tensor_product": [c_int, _P, _P, c_int64, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int32), _P, ctypes.POINTER(ctypes.c_int32),
                           c_int, _P, c_int64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(c_double), _P, _P],
    "xeq_tensor_product_wgrad": [c_int, _P, _P, _P, c_int64, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int32), _P,
                                 ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), c_int,
                                 ctypes.POINTER(c_double), c_int, _P, _P],
    "xeq_tensor_product_wgrad_chunks": [c_int64],
    "xeq_tensor_product_form": [c_int, c_int64, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int32), c_int],
    "xeq_scatter_add": [c_int, _P, _P, c_int64, c_int64, _P, c_int64, _P],
    "xeq_message_fwd": [c_int, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                        c_int, c_int, c_int, c_double, c_int, _I3, _P, _P, c_int, _P],
    "xeq_message_bwd": [c_int, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                        c_int, c_int, c_int, c_double, c_int, _I3, _P, _P, _P, c_int, _P],
    "xeq_message_param_grad_parts": [c_int64],
    "xeq_message_param_grad": [c_int, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_double, c_int,
                               _I3, c_int, c_int, _P, _P],
    "xeq_message_param_grad_mc_supported": [c_int, c_int, c_int, c_int, _I3],
    "xeq_param_basis_width": [c_int, c_int],
    "xeq_message_param_grad_mc_parts": [c_int64, c_int, _I3],
    "xeq_param_basis": [_P, c_int64, c_int, c_int, c_int, c_double, _P, _P, _P, _P],
    "xeq_message_param_grad_mc": [c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _I3, c_int, c_int, _P, c_int, _P, _P],
    "xeq_to_bt": [_P, c_int64, _I3, _P, _P],
    "xeq_norm_param_grad_chunks": [c_int64],
    "xeq_norm_param_grad": [_P, _P, _P, _P, c_int64, _P, c_int64, c_int, _I3, c_int, _P, _P],
    "xeq_message_auto_family": [c_int, c_int64, c_int64, c_int, c_int, _I3],
    "xeq_message_wq_edges_per_stream": [c_int64, c_int64],
    "xeq_edge_basis_width": [c_int],
    "xeq_edge_basis": [c_int, _P, c_int64, c_int, c_int, c_int, c_double, _P, _P, _P, _P, _P],
    "xeq_message_fwd_sb": [c_int, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, _I3, _P, _P, c_int, _P],
    "xeq_message_bwd_sbq": [c_int, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, _I3, _P, _P, _P, _P, c_int, _P],
    "xeq_message_q_wgrad": [c_int, _P, _P, c_int64, c_int, c_int, _I3, c_int, _P, _P],
    "xeq_message_q_wgrad_chunks": [c_int64],
    "xeq_train_norm": [c_int, c_int, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _I3, c_double, c_double, c_int, _P, _P, _P, _P],
    "xeq_train_uv": [c_int, c_int, c_int64, _P, _P, _P, _I3, c_double, _P, _P, _P],
    "xeq_train_out": [c_int, c_int, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _I3, _P, _P, _P, _P],
    "xeq_train_edge_supported": [c_int, c_int, c_int, c_int],
    "xeq_train_edge": [c_int, c_int, c_int64, _P, _P, _P, _P, c_int, c_int, c_int, c_double, _P, _P, _P, _P],
    "xeq_zero_rows_from": [_P, c_int64, c_int64, _P, _P],
    "xeq_message_fwd_sb_pair": [c_int, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, _I3, _P, _P, c_int, _P],
    "xeq_message_bwd_sbq_pair": [c_int, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, _I3, _P, _P, _P, _P, c_int, _P],
    "xeq_message_bwd_sb": [c_int, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, _I3, _P, _P, _P,
                           c_int, _P],
    "xeq_message_sb_fits": [c_int64, c_int64, c_int, c_int, _I3],
    "xeq_message_wq_supported": [c_int, c_int, _I3],
    "xeq_message_wq_fits": [c_int64, c_int64, c_int, c_int, _I3],
    "xeq_message_wq_pcap": [c_int64, c_int64],
    "xeq_message_wq_waves": [],
    "xeq_message_wq_record_floats": [],
    "xeq_message_wq_record_floats_for": [c_int],
    "xeq_message_wq_plan_workspace": [c_int64],
    "xeq_message_wq_win_ints": [c_int],
    "xeq_message_wq_plan": [_P, _P, _P, _P, c_int64, c_int64, c_int, _P, c_int64, _P, _P, _P, _P, _P, _P, _P, _P],
    "xeq_edge_basis_wq": [_P, c_int64, c_int64, _P, _P, c_int, c_int, c_int, c_double, _P, _P, _P, _P, _P],
    "xeq_message_fwd_wq": [c_int64, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, _I3,
                           _P, _P, c_int, _P],
    "xeq_message_wq_table_max_rows": [],
    "xeq_message_wq_first_table": [c_int, c_int64, c_int, c_int],
    "xeq_edge_basis_wq_table": [_P, c_int64, c_int64, _P, _P, c_int, c_int, c_int, c_double, _P, _P, _P, _P, _P, _P, _P, c_int, c_int64, _P, _P, _P],
    "xeq_message_fwd_wq_table": [c_int64, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, _P, _P, _P, _P, c_int, c_int, _I3,
                                 _P, _P, c_int, _P],
    "xeq_message_bwd_wq_table": [c_int64, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, _P, _P, _P, _P, c_int, c_int,
                                 _I3, _P, c_int, _P],
    "xeq_message_wq_parts_floats": [c_int64, c_int64, _I3],
    "xeq_message_bwd_wq": [c_int64, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int,
                           _I3, _P, _P, _P, c_int, _P],
    "xeq_message_wq_packed_weight_floats": [c_int, c_int, _I3],
    "xeq_message_wq_pack_weights": [_P, _P, c_int, c_int, _I3, _P, _P],
    "xeq_message_wq_edge_grad": [_P, c_int64, c_int64, _P, _P, _P, _I3, _P, _P, _P],
    "xeq_message_wq_edge_grad_sum": [_P, c_int64, c_int64, _P, _P, _P, _I3, c_int, ctypes.POINTER(c_void_p), _P, _P],
    "xeq_norm_fwd": [c_int, _P, _P, _P, _P, _P, _P, c_int64, c_int, _I3, c_int, _P, c_int64, _P, _P, _P],
    "xeq_norm_bwd": [c_int, _P, _P, _P, _P, _P, c_int64, c_int, _I3, c_int, _P, c_int64, _P, _P, _P, _P, _P, _P],
    "xeq_uv_reduce_fwd": [c_int, _P, c_int64, _I3, c_double, _P, c_int64, c_int, _P, _P],
    "xeq_uv_reduce_bwd": [c_int, _P, _P, _P, c_int64, c_int, c_int64, _I3, c_double, _P, _P, _P, _P],
    "xeq_update_out_fwd": [c_int, _P, _P, _P, _P, _P, c_int64, c_int, _I3, _P, _P, _P],
    "xeq_update_out_bwd": [c_int, _P, _P, _P, _P, _P, c_int64, c_int, _I3, _P, _P, _P, _P],
    "xeq_update_uv_supported": [c_int, c_int, _I3],
    "xeq_update_uv_fwd": [_P, _P, _P, _P, _P, _P, c_int64, c_int, _I3, c_int, _P, _P, _P, c_int, c_double, _P, c_int64, _P, _P, _P, _P],
    "xeq_update_uv_bwd": [_P, _P, _P, c_int64, _P, _P, _P, c_int64, _P, _P, _P, _P, _P, c_int64, c_int, _I3, c_int, _P, _P, _P, c_double,
                          _P, _P, _P, _P],
    "xeq_mlp2_supported": [c_int, c_int, c_int, c_int],
    "xeq_node_tile_split": [c_int64, c_int, ctypes.POINTER(c_int64)],
    "xeq_mlp_packed_floats": [c_int, c_int],
    "xeq_mlp_pack": [_P, _P, c_int, c_int, c_int, _P, _P],
    "xeq_mlp2_fwd": [_P, c_int64, c_int64, c_int, _P, _P, c_int, _P, _P, c_int64, _P],
    "xeq_mlp2_bwd": [_P, c_int64, c_int64, c_int, _P, _P, _P, c_int, _P, c_int64, _P],
    "xeq_mlp2h_supported": [c_int, c_int, c_int, c_int],
    "xeq_mlp2h_fwd": [c_int, _P, c_int64, c_int64, c_int, c_int, _P, _P, c_int, _P, _P, c_int64, _P],
    "xeq_mlp2h_bwd": [c_int, _P, c_int64, c_int64, c_int, c_int, _P, _P, _P, c_int, _P, c_int64, _P],
    "xeq_mlp2_and_linear": [c_int, _P, c_int64, c_int64, c_int, _P, _P, c_int, _P, _P, c_int64, _P, c_int64, c_int, _P, c_int, _P, c_int64, _P],
    "xeq_pack_epoch": [],
    "xeq_pack_epoch_bump": [],
    "xeq_rowptr_guard": [_P, c_int64, c_int64, _P, _P, _P],
    "xeq_node_block_supported": [c_int, c_int, _I3],
    "xeq_node_block_fwd_tiles": [c_int],
    "xeq_node_block_rows": [c_int64],
    "xeq_node_block_auto": [c_int64],
    "xeq_small_rows_limit": [],
    "xeq_node_block_set_waves": [c_int],
    "xeq_node_block_pack_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "xeq_node_block_fwd": [c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                           _P, _P, _P, _P, _P],
    "xeq_node_block_linear_test": [_P, c_int64, _P, c_int, c_int, _P, _P, _P],
    "xeq_node_block_bwd_tiles": [c_int, c_int],
    "xeq_node_block_pack_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, _P],
    "xeq_node_block_bwd": [c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_double, _P, _P, _P, _P, _P,
                           _P, _P, _P],
    "xeq_painn_supported": [c_int, c_int, c_int],
    "xeq_painn_few_rows_limit": [],
    "xeq_painn_filter_packed_floats": [c_int],
    "xeq_painn_uv_packed_floats": [c_int],
    "xeq_painn_pack_filter": [_P, _P, c_int, c_int, _P, _P],
    "xeq_painn_pack_uv": [_P, _P, c_int, _P, _P],
    "xeq_painn_message_fwd": [c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_double, c_int, _P, _P, _P],
    "xeq_painn_message_bwd": [c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_double, c_int, _P, _P, _P, _P, _P,
                              c_int, _P],
    "xeq_painn_update_uv_fwd": [c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P],
    "xeq_painn_update_out_fwd": [c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P],
    "xeq_painn_update_out_bwd": [c_int64, c_int, _P, _P, _P, _P, _P, _P],
    "xeq_painn_update_uv_bwd": [c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "xeq_painn_add": [_P, _P, c_int64, _P, _P],
    "xeq_head_polar_supported": [c_int, c_int, c_int, c_int, c_int, c_int, c_int],
    "xeq_head_polar_nodes": [_P, c_int64, _P, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P,
                             c_double, _P, _P],
    "xeq_head_graph_reduce": [c_int, _P, c_int64, c_int, _P, c_int64, _P, _P, _P, _P],
    "xeq_ewald_supported": [c_int, c_int, c_int],
    "xeq_ewald_chunk": [],
    "xeq_ewald_parts_floats": [c_int64, c_int64, c_int, c_int],
    "xeq_ewald_structure_factor": [_P, c_int64, c_int64, c_int, _P, _P, c_int64, c_int, _P, _P, c_int64, _P, _P, _P, _P],
    "xeq_ewald_apply": [_P, _P, _P, c_int64, c_int, _P, _P, c_int64, c_int, _P, _P, c_int64, _P, c_int64, _P],
    "xeq_ewald_phase_grad": [_P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, c_int64, c_int, _P, _P, c_int64, c_int, _P, _P, _P, c_int64, _P, _P, _P, _P],
    "xeq_ewald_damping": [_P, c_int64, c_double, c_double, _P, _P, _P],
    "xeq_ewald_layernorm_fwd": [_P, c_int64, c_int, _P, _P, c_double, _P, _P, _P],
    "xeq_ewald_layernorm_bwd": [_P, _P, _P, _P, c_int64, c_int, _P, _P],
    "xeq_ewald_combine": [_P, c_double, _P, c_double, _P, c_int64, _P, _P],
    "xeq_record_bytes": [c_int],
    "xeq_md_inverse_cell": [ctypes.POINTER(c_double), ctypes.POINTER(c_double)],
    "xeq_md_normals": [c_int, c_uint64, c_int, c_uint64, _P, c_int64, _P, _P, _P],
    "xeq_md_front": [_R(ResSystem), _R(MdParams), c_double, _P],
    "xeq_md_back": [_R(ResSystem), _R(ResStep), _R(ResChunks), _R(MdParams), _R(ResRecorder), c_int, _P],
    "xeq_pbc_tables_device": [c_int, _P, _I3, _I3, c_double, _P, c_int64, _P, _P],
    "xeq_npt_front": [_R(ResSystem), _R(MdParams), _R(NptParams), c_double, _P],
    "xeq_npt_back": [_R(ResSystem), _R(ResStep), _R(ResChunks), _R(MdParams), _R(NptParams), _R(ResRecorder), c_int, _P],
    "xeq_nvt_front": [_R(ResSystem), _R(MdParams), _R(NvtParams), c_double, _P],
    "xeq_nvt_back": [_R(ResSystem), _R(ResStep), _R(ResChunks), _R(MdParams), _R(NvtParams), _R(ResRecorder), c_int, _P],
    "xeq_fire_front": [_R(ResSystem), _R(FireParams), _P],
    "xeq_fire_back": [_R(ResSystem), _R(ResStep), _R(ResChunks), _R(FireParams), _R(ResRecorder), _P],
    "xeq_lbfgs_front": [_R(ResSystem), _R(ResChunks), _R(LbfgsParams), _P],
    "xeq_lbfgs_back": [_R(ResSystem), _R(ResStep), _R(ResChunks), _R(LbfgsParams), _R(ResRecorder), _P],
    "xeq_vib_project": [c_int, _P, _P, _P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "xeq_vib_eigh": [_P, _P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P],
    "xeq_vib_eigh_large": [_P, _P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P],
    "xeq_vib_finish": [_P, _P, _P, _P, _P, c_int64, _P, _P, _P, c_double, c_double, _P, _P, _P, _P, _P, _P, _P, _P],
    "xeq_vib_thermo_sums": [_P, _P, _P, c_int64, c_double, _P, _P],
}
# entry points that return a size, not a status
_RET_I64 = {"xeq_record_bytes", "xeq_launch_count", "xeq_launch_names", "xeq_message_wq_packed_weight_floats", "xeq_rowptr_from_degrees_max", "xeq_csr_by_key_workspace", "xeq_message_wq_pcap", "xeq_message_wq_plan_workspace", "xeq_message_wq_win_ints",
            "xeq_message_wq_parts_floats", "xeq_mlp_packed_floats", "xeq_exclusive_scan_i32_workspace", "xeq_node_block_fwd_tiles", "xeq_node_block_bwd_tiles", "xeq_node_block_rows", "xeq_pack_epoch", "xeq_tensor_product_wgrad_chunks", "xeq_small_rows_limit", "xeq_painn_few_rows_limit",
            "xeq_painn_filter_packed_floats", "xeq_painn_uv_packed_floats", "xeq_ewald_chunk", "xeq_ewald_parts_floats"}
EXPORTS = ["xeq_version", "xeq_last_error", *_PROTOS]

_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    """dlopen the in-tree HIP library (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -m xequinet_amd.csrc.build` "
            "(xequinet_amd has no CPU / pure-PyTorch fallback)"
        )
    lib = ctypes.CDLL(LIB_PATH)
    lib.xeq_version.restype = c_int
    lib.xeq_last_error.restype = c_char_p
    for name, argtypes in _PROTOS.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = c_int64 if name in _RET_I64 else c_int
    for which, record in [*enumerate(RECORDS), *RECORDS_APART.items()]:      # a binding whose layout is not the library's would hand kernels the wrong buffers
        if ctypes.sizeof(record) != lib.xeq_record_bytes(which):
            raise ImportError(f"{LIB_PATH}: {record.__name__} is {lib.xeq_record_bytes(which)} bytes in the library, {ctypes.sizeof(record)} in "
                              "xequinet_amd/lib.py (a library of another version?)")
    _lib = lib
    return lib


def pack_epoch() -> int:
    """Epoch of the packed weight copies (include/xeq.h): part of every pack-cache key."""
    return int(load().xeq_pack_epoch())


def bump_pack_epoch() -> None:
    """Parameters changed behind autograd's back (a replayed captured optimizer step): every pack cache misses from here on."""
    load().xeq_pack_epoch_bump()


def pack_key(tensors, extra=()) -> tuple:
    """THE key of a packed copy: (version counter, address) of every tensor it was made from (None for an absent one), the flags that
    select its form, the pack epoch.  An in-place update moves the version, a replaced storage the address, a replayed captured
    optimizer step the epoch."""
    return (*[None if t is None else (t._version, t.data_ptr()) for t in tensors], *extra, pack_epoch())


def cached(owner, slot: str, tensors, build, extra=()):
    """What ``build()`` (run under no_grad) returned last for ``pack_key(tensors, extra)``, kept on ``owner`` as the attribute
    ``slot`` = (key, value).  Every packed-weight cache of the Python front is this function."""
    key = pack_key(tensors, extra)
    hit = getattr(owner, slot, None)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        value = build()
    setattr(owner, slot, (key, value))
    return value


def launch_count() -> int:
    """Kernel launches libxeq_hip.so has enqueued in this process (include/xeq.h: xeq_launch_count)."""
    return int(load().xeq_launch_count())


def launch_names(first: int) -> list:
    """Entry-point names of the launches numbered ``first`` .. launch_count() - 1, in order (include/xeq.h: xeq_launch_names)."""
    L = load()
    need = int(L.xeq_launch_names(int(first), None, 0))
    if need < 0:
        raise ValueError("launch_names: the range is out of the library's ring of names")
    buf = ctypes.create_string_buffer(need)
    L.xeq_launch_names(int(first), buf, need)
    return [n for n in buf.value.decode().split("\n") if n]


def call(name: str, *args) -> None:
    lib = load()
    status = getattr(lib, name)(*args)
    if status != 0:
        raise RuntimeError(f"{name} failed ({status}): {lib.xeq_last_error().decode()}")


def dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return XEQ_F32
    if t.dtype == torch.float64:
        return XEQ_F64
    raise TypeError(f"xequinet_amd supports float32/float64 tensors, got {t.dtype}")


def require_hip(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "xequinet_amd ops run on MI355X (HIP) tensors only and have no CPU fallback; "
                f"got a tensor on {t.device}"
            )


def ptr3(ts):
    """Three device pointers as one argument (``const void* const [3]``); None for an absent list."""
    if ts is None:
        return None
    return (c_void_p * 3)(*[None if t is None else t.data_ptr() for t in ts])


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else c_void_p(t.data_ptr())


def stream() -> c_void_p:
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def mul3(mul) -> ctypes.Array:
    return (c_int32 * 3)(*[int(m) for m in mul])
