"""ctypes mirror of include/fea_hip.h and host/fea_host.h.

Python is plumbing here (tests, bench): every call goes straight through the
C ABI of libfeahip.so -- the same symbols a C host (the reference's solve(),
solver-large/fea_solver.c:130-242) binds.  There is no Python or CPU
implementation behind these names: if the shared library is missing, or no
HIP device is visible, construction fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FEAHIP_LIB: measurement tooling only (the diagnostic build libfeahip_dbg.so); still a HIP library, never a fallback
LIB_PATH = os.environ.get("FEAHIP_LIB") or os.path.join(_HERE, "libfeahip.so")
HOST_LIB_PATH = os.path.join(_HERE, "libfeahost.so")

MODEL_A5, MODEL_COMPRESSIBLE_NEOHOOKEAN = 0, 1
CG, PCG_ILU, CHOLESKY = 0, 1, 2
EINVAL, ESTATE, ENOTCONVERGED = -1, -5, -6              # FEAHIP_E* of include/fea_hip.h
ASM_AUTO, ASM_ROWOWNER, ASM_ATOMIC, ASM_PATCH, ASM_STAGED, ASM_PAIRED, ASM_PIPELINED, ASM_SHARED, ASM_GATHER = 0, 1, 2, 3, 4, 5, 6, 7, 8
TETRAHEDRA10, TETRAHEDRA4, HEXAHEDRA8 = 0, 1, 2
LOAD_PRESSURE, LOAD_TRACTION = 0, 1

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

# every symbol include/fea_hip.h declares, with its argument types
ABI = {
    "feahip_create": [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip, _dp,
                      C.c_int, _dp, C.c_int, C.c_int, _ip, _ip, _dp],
    "feahip_destroy": [C.c_void_p],
    "feahip_last_error": [C.c_void_p],
    "feahip_create_error": [],
    "feahip_update_nodes_with_bc": [C.c_void_p, C.c_double],
    "feahip_update_state": [C.c_void_p, _ip],
    "feahip_create_stiffness": [C.c_void_p],
    "feahip_create_residual_forces": [C.c_void_p],
    "feahip_create_stiffness_and_residual": [C.c_void_p],
    "feahip_stash_stiffness": [C.c_void_p],
    "feahip_restore_stiffness": [C.c_void_p],
    "feahip_apply_prescribed_bc": [C.c_void_p, C.c_double],
    "feahip_solve_slae": [C.c_void_p, C.c_int, C.c_double, C.c_int, _ip, _dp],
    "feahip_solve_slae2": [C.c_void_p, C.c_int, C.c_double, C.c_int, _dp, _ip, _dp],
    "feahip_get_solution2": [C.c_void_p, _dp],
    "feahip_spmv2": [C.c_void_p, _dp, _dp],
    "feahip_solve_arclength": [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, _dp, _dp,
                               C.c_int, _ip, _ip],
    "feahip_energy": [C.c_void_p, _dp],
    "feahip_update_nodes_with_solution": [C.c_void_p, _dp],
    "feahip_solve": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, _dp,
                     C.c_int, _ip, _ip],
    "feahip_set_nodes": [C.c_void_p, _dp],
    "feahip_get_nodes": [C.c_void_p, _dp],
    "feahip_get_forces": [C.c_void_p, _dp],
    "feahip_set_forces": [C.c_void_p, _dp],
    "feahip_get_solution": [C.c_void_p, _dp],
    "feahip_get_graddefs": [C.c_void_p, _dp],
    "feahip_get_stresses": [C.c_void_p, _dp],
    "feahip_get_shape_gradients": [C.c_void_p, _dp, _dp],
    "feahip_matrix_nnz": [C.c_void_p, C.POINTER(C.c_longlong)],
    "feahip_get_matrix_yale": [C.c_void_p, _ip, _ip, _dp],
    "feahip_get_matrix_yale64": [C.c_void_p, C.POINTER(C.c_longlong), _ip, _dp],
    "feahip_spmv": [C.c_void_p, _dp, _dp],
    "feahip_set_assembly": [C.c_void_p, C.c_int],
    "feahip_set_preconditioner": [C.c_void_p, C.c_int],
    "feahip_set_line_search": [C.c_void_p, C.c_int],
    "feahip_set_pcg_variant": [C.c_void_p, C.c_int],
    "feahip_set_row_shard": [C.c_void_p, C.c_int, C.c_int],
    "feahip_comm_unique_id": [C.c_void_p, C.c_int],
    "feahip_comm_init": [C.c_void_p, C.c_int, C.c_int, C.c_void_p],
    "feahip_owned_rows": [C.c_void_p, _ip, _ip],
    "feahip_group_init": [C.POINTER(C.c_void_p), C.c_int],
    "feahip_group_solve_slae": [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_double, C.c_int, _ip, _dp],
    "feahip_group_energy": [C.POINTER(C.c_void_p), C.c_int, _dp],
    "feahip_group_update_nodes_with_solution": [C.POINTER(C.c_void_p), C.c_int],
    "feahip_group_solve": [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                           C.c_double, C.c_int, _dp, C.c_int, _ip, _ip],
    "feahip_shard_plan": [C.c_int, C.c_int, C.c_int, _ip, C.c_int, C.c_int, _ip, _ip, _ip, _ip, _ip, _ip],
    "feahip_sync": [C.c_void_p],
    "feahip_time_kernel": [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp],
    "feahip_sizes": [C.c_void_p, C.POINTER(C.c_longlong)],
    "feahip_host_gather_stats": [C.c_int, C.c_int, C.c_int, _ip, C.POINTER(C.c_longlong), _ip],
    "feahip_host_gather10_shape": [C.c_int, C.c_int, C.c_int, _ip, C.POINTER(C.c_longlong)],
    "feahip_host_gather_chunks": [C.c_int, C.c_int, _ip, C.c_int, _ip],
    "feahip_host_gather_walk": [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int, _ip, _ip, _ip,
                                C.c_longlong, C.c_void_p],
    "feahip_host_assembly_digest": [C.c_int, C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.POINTER(C.c_ulonglong), _ip],
    "feahip_assembly_in_use": [C.c_void_p, _ip],
    "feahip_node_numbering": [C.c_void_p, _ip],
    "feahip_create_rank": [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip, _dp,
                           C.c_int, _dp, C.c_int, C.c_int, _ip, _ip, _dp],
    "feahip_create_rank_local": [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, _dp, _dp, _ip, _dp, _ip, _ip, _ip, C.c_int, _dp, C.c_int, C.c_int, _ip, _ip, _dp],
    "feahip_host_rank_local_plan": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _ip, _ip, _ip, _ip, _ip,
                                    _ip, _ip],
    "feahip_host_slab_order": [C.c_int, C.c_int, C.c_int, C.c_int, _ip, _dp, _ip],
    "feahip_rank_counts": [C.c_void_p, C.POINTER(C.c_longlong)],
    "feahip_rank_maps": [C.c_void_p, _ip, _ip],
    "feahip_host_rank_plan": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _dp, _ip, _ip, _ip, _ip, _ip, _ip],
    "feahip_host_rank_mesh": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _dp, C.POINTER(C.c_longlong), _ip, _ip,
                              C.POINTER(C.c_longlong), _ip],
    "feahip_copy_bandwidth": [C.c_void_p, C.c_longlong, _dp],
    "feahip_copy_bandwidth_detail": [C.c_void_p, C.c_longlong, _dp],
    "feahip_assembly_stats": [C.c_void_p, _dp],
    "feahip_device_layout": [C.c_void_p, C.POINTER(C.c_longlong)],
    "feahip_host_numbering": [C.c_int, C.c_int, C.c_int, _ip, _dp, _ip],
    "feahip_set_surface_loads": [C.c_void_p, C.c_int, C.c_int, _ip, _ip, _dp],
    "feahip_get_surface_forces": [C.c_void_p, _dp],
    "feahip_set_contact": [C.c_void_p, C.c_int, C.c_int, _ip, C.c_int, _ip, _dp, C.c_double, C.c_int, C.c_double],
    "feahip_get_contact_nodes": [C.c_void_p, _ip, _ip, _dp],
    "feahip_get_contact_obstacles": [C.c_void_p, _ip],
    "feahip_get_contact_multipliers": [C.c_void_p, _dp],
    "feahip_set_contact_multipliers": [C.c_void_p, _dp],
    "feahip_get_contact_forces": [C.c_void_p, _dp],
    "feahip_get_contact_status": [C.c_void_p, _dp, _dp],
    "feahip_contact_info": [C.c_void_p, _dp],
    "feahip_contact_augment": [C.c_void_p, _dp],
    "feahip_set_load_factor": [C.c_void_p, C.c_double],
    "feahip_get_load_factor": [C.c_void_p, _dp],
    "feahip_set_materials": [C.c_void_p, C.c_int, _dp, _ip],
    "feahip_get_materials": [C.c_void_p, _ip, _dp, _ip],
    "feahip_host_surface_faces": [C.c_int, C.c_int, C.c_int, _ip, C.c_int, C.c_int, _ip, _ip, _ip, _ip],
    "feahip_apply_preconditioner": [C.c_void_p, _dp, _dp],
    "feahip_amg_info": [C.c_void_p, C.POINTER(C.c_longlong), _dp],
    "feahip_amg_level": [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), _dp, _ip, _ip, _dp, _ip, _dp, _ip],
    "feahip_group_apply_preconditioner": [C.POINTER(C.c_void_p), C.c_int, C.POINTER(_dp), C.POINTER(_dp)],
    "feahip_coarse_info": [C.c_void_p, C.POINTER(C.c_longlong), _ip, _dp],
    "feahip_coarse_matrix": [C.c_void_p, _dp],
    "feahip_host_coarse_aggregates": [C.c_int, C.c_int, _ip],
    "feahip_set_mass": [C.c_void_p, C.c_int, _dp, C.c_int, _dp, _dp, _dp],
    "feahip_mass_spmv": [C.c_void_p, _dp, _dp],
    "feahip_set_body_force": [C.c_void_p, _dp],
    "feahip_set_damping": [C.c_void_p, C.c_double, C.c_double],
    "feahip_get_damping": [C.c_void_p, _dp, _dp],
    "feahip_damping_spmv": [C.c_void_p, _dp, _dp],
    "feahip_host_rayleigh": [C.c_double, C.c_double, C.c_double, C.c_double, _dp, _dp],
    "feahip_set_velocities": [C.c_void_p, _dp],
    "feahip_get_velocities": [C.c_void_p, _dp],
    "feahip_set_accelerations": [C.c_void_p, _dp],
    "feahip_get_accelerations": [C.c_void_p, _dp],
    "feahip_get_time": [C.c_void_p, _dp],
    "feahip_set_time": [C.c_void_p, C.c_double],
    "feahip_consistent_acceleration": [C.c_void_p, C.c_int, C.c_double, C.c_int],
    "feahip_solve_dynamic": [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int,
                             C.c_double, C.c_int, _dp, C.c_int, _ip, _ip],
    "feahip_group_solve_dynamic": [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                   C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, _dp, C.c_int, _ip, _ip],
    "feahip_get_lumped_mass": [C.c_void_p, _dp],
    "feahip_stable_step": [C.c_void_p, _dp],
    "feahip_kinetic_energy": [C.c_void_p, _dp],
    "feahip_solve_explicit": [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, _dp, C.c_int, _ip],
    "feahip_group_solve_explicit": [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, _dp,
                                    C.c_int, _ip],
    "feahip_get_nodal_stresses": [C.c_void_p, C.c_int, _dp, _dp, _dp],
    "feahip_strain_energy": [C.c_void_p, _dp],
    "feahip_get_nodal_energy": [C.c_void_p, _dp],
    "feahip_get_reactions": [C.c_void_p, _dp],
    "feahip_solve_modes": [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, _dp, _dp, _ip],
    "feahip_get_modes": [C.c_void_p, C.c_int, C.c_int, _dp],
    "feahip_spmm_km": [C.c_void_p, _dp, _dp, _dp],
    "feahip_solve_modes_sharded": [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, _dp, _dp, _ip],
    "feahip_group_spmm_km": [C.POINTER(C.c_void_p), C.c_int, C.POINTER(_dp), C.POINTER(_dp), C.POINTER(_dp)],
    "feahip_host_modal_ritz": [C.c_int, _dp, _dp, _dp, _dp],
    "feahip_solve_modes_locked": [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, _dp, _dp, _ip, _ip],
    "feahip_get_locked_modes": [C.c_void_p, C.c_int, C.c_int, _dp],
    "feahip_get_locked_count": [C.c_void_p, _ip],
    "feahip_get_locked_lambda": [C.c_void_p, C.c_int, C.c_int, _dp],
    "feahip_modal_deflate": [C.c_void_p, C.c_int, _dp, _dp, _dp],
    "feahip_response_set_basis": [C.c_void_p, C.c_int, _dp, _dp],
    "feahip_response_load": [C.c_void_p, _dp, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _ip, _dp],
    "feahip_get_response_static": [C.c_void_p, _dp],
    "feahip_response_sweep": [C.c_void_p, C.c_int, _dp, C.c_double, C.c_double, _dp, _dp, _ip, C.c_int, _ip, _dp, _dp],
    "feahip_response_field": [C.c_void_p, C.c_double, C.c_double, C.c_double, _dp, _dp, _dp],
    "feahip_host_response_coefficients": [C.c_int, _dp, _dp, C.c_int, _dp, C.c_double, C.c_double, _dp, C.c_int, _dp],
    "feahip_response_base_load": [C.c_void_p, _dp, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _ip, _dp],
    "feahip_response_transient": [C.c_void_p, C.c_int, C.c_double, _dp, C.c_double, C.c_double, _dp, C.c_int, _dp, _ip,
                                  C.c_int, _ip, _dp, C.c_int, _ip, _dp],
    "feahip_host_transient_coefficients": [C.c_int, _dp, _dp, C.c_int, C.c_double, _dp, C.c_double, C.c_double, _dp, C.c_int,
                                           C.c_int, _dp],
    "feahip_response_combine": [C.c_void_p, _dp, _dp, C.c_double, C.c_int, _dp],
    "feahip_response_random": [C.c_void_p, C.c_int, _dp, _dp, C.c_double, C.c_double, _dp, C.c_int, _dp, _dp],
    "feahip_response_spectrum": [C.c_void_p, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, C.c_double, _dp, C.c_double,
                                 C.c_int, _dp, _dp],
    "feahip_stress_increment": [C.c_void_p, _dp, C.c_int, _dp],
    "feahip_response_stress_basis": [C.c_void_p, C.c_int],
    "feahip_get_modal_stresses": [C.c_void_p, C.c_int, C.c_int, _dp],
    "feahip_get_response_static_stress": [C.c_void_p, _dp],
    "feahip_response_stress_field": [C.c_void_p, _dp, C.c_double, _dp, _dp],
    "feahip_response_stress_combine": [C.c_void_p, _dp, _dp, C.c_double, _dp, _dp],
    "feahip_response_stress_random": [C.c_void_p, C.c_int, _dp, _dp, C.c_double, C.c_double, _dp, _dp, _dp, _dp],
    "feahip_response_stress_spectrum": [C.c_void_p, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, C.c_double, _dp, C.c_double,
                                        _dp, _dp, _dp],
    "feahip_response_stress_sweep": [C.c_void_p, C.c_int, _dp, C.c_double, C.c_double, _dp, _dp, _ip, _dp, _ip, C.c_int, _ip,
                                     _dp, _dp],
    "feahip_response_stress_transient": [C.c_void_p, C.c_int, C.c_double, _dp, C.c_double, C.c_double, _dp, _dp, _ip, _dp, _ip,
                                         C.c_int, _ip, _dp],
    "feahip_host_harmonic_von_mises": [_dp, _dp],
    "feahip_host_random_form": [C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_double, C.c_double, _dp, C.c_int, C.c_int, _dp, _dp,
                                _dp],
    "feahip_host_random_grid": [C.c_int, _dp, C.c_double, C.c_double, _dp, C.c_double, C.c_double, C.c_int, C.c_int, _dp, _ip],
    "feahip_host_psd_value": [C.c_int, _dp, _dp, C.c_int, C.c_double],
    "feahip_host_spectrum_value": [C.c_int, _dp, _dp, C.c_int, C.c_double],
    "feahip_host_spectrum_form": [C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, _dp, C.c_int, C.c_int, C.c_double, C.c_int,
                                  _dp, _dp, _dp],
    "feahip_host_moment_form": [C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_double, C.c_double, _dp, C.c_int, C.c_int, _dp, _dp,
                                _dp],
    "feahip_host_fatigue": [C.c_int, _dp, C.c_double, C.c_double, _dp, _dp, _ip],
    "feahip_response_stress_moments": [C.c_void_p, _dp, _dp, _dp, _dp],
    "feahip_response_stress_fatigue": [C.c_void_p, C.c_int, _dp, _dp, C.c_double, C.c_double, _dp, C.c_double, C.c_double, _dp,
                                       _dp, _dp, _ip],
    "feahip_host_rainflow": [C.c_int, _dp, C.c_double, C.c_double, C.c_int, _dp, _dp, _dp, _ip, _ip, C.c_int, _ip, _dp, _dp, _dp],
    "feahip_response_stress_rainflow": [C.c_void_p, C.c_int, C.c_double, _dp, C.c_double, C.c_double, _dp, C.c_double, C.c_double,
                                        C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip, C.c_int, _ip, _dp],
    "feahip_solve_buckling": [C.c_void_p, C.c_int, C.c_double, C.c_int, _dp, _dp, _dp, _ip],
    "feahip_get_buckling_modes": [C.c_void_p, C.c_int, C.c_int, _dp],
    "feahip_geometric_spmv": [C.c_void_p, _dp, _dp],
    "feahip_host_buckling_factor": [C.c_int, _dp, _dp],
}
MODAL_COLS = 8                                          # FEA_MODAL_COLS of include/fea_hip.h
MODAL_MAX_LOCKED = 64                                   # FEA_MODAL_MAX_LOCKED
RESPONSE_MAX_FREQ = 4096                                # FEA_RESPONSE_MAX_FREQ
TRANSIENT_MAX_STEPS = 1048576                           # FEA_TRANSIENT_MAX_STEPS
TRANSIENT_CHUNK = 8064                                  # FEA_TRANSIENT_CHUNK
TRANSIENT_SHAPES = ("step", "ramp", "half-sine")        # FEA_SHAPE_* of host/fea_host.h
RANDOM_MAX_FREQ = 262144                                # FEA_RANDOM_MAX_FREQ
DECK_MAX_POINTS = 4096                                  # FEA_DECK_MAX_POINTS of host/fea_host.h
SPECTRUM_RULES = ("srss", "cqc", "abs")                 # :rule of (spectrum ...), the values of FEAHIP_SRSS, _CQC, _ABS
SRSS, CQC, ABS = 0, 1, 2                                # FEAHIP_SRSS, FEAHIP_CQC, FEAHIP_ABS: the rules of a response spectrum
# the mass rule FeaSolver.set_mass picks (exact for straight-sided elements; fea_mass_points of host/fea_host.h)
MASS_POINTS = {TETRAHEDRA4: 4, TETRAHEDRA10: 27, HEXAHEDRA8: 8}
COARSE_INFO_KEYS = ("aggregates", "first_aggregate", "local_aggregates", "unknowns", "epoch", "owned_rows", "m", "pairs")
AMG_INFO_KEYS = ("levels", "gamma", "gamma_from", "gamma_until", "coarse_sweeps", "fine_bits", "coarse_f32", "fused_post",
                 "tail_from", "tail_entry", "tail_cop", "tail_lds_levels", "row0", "row1", "tail_blob")
TAIL_ENTRY = {0: None, 1: "lds", 2: "ell", 3: "l2"}

_lib = None
_host = None


class FeaHipError(RuntimeError):
    pass


def load_library():
    """dlopen libfeahip.so and type every ABI symbol (no device is touched)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FeaHipError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`; "
                "there is no fallback implementation")
        lib = C.CDLL(LIB_PATH)
        for name, args in ABI.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is absent
            fn.argtypes = args
            fn.restype = C.c_char_p if name in ("feahip_last_error", "feahip_create_error") else (
                None if name == "feahip_destroy" else
                C.c_double if name in ("feahip_host_psd_value", "feahip_host_spectrum_value",
                                       "feahip_host_harmonic_von_mises") else C.c_int)
        _lib = lib
    return _lib


class FeaDeck(C.Structure):
    """struct fea_deck of host/fea_host.h."""
    _fields_ = [
        ("model", C.c_int), ("parameters", C.c_double * 10), ("parameters_count", C.c_int),
        ("solver_type", C.c_int), ("solver_tolerance", C.c_double), ("solver_max_iter", C.c_int),
        ("ele_type", C.c_int), ("load_increments_count", C.c_int), ("desired_tolerance", C.c_double),
        ("max_newton_count", C.c_int), ("linesearch_max", C.c_int), ("arclength_max", C.c_int),
        ("modified_newton", C.c_int), ("nodes_per_element", C.c_int), ("gauss_nodes_count", C.c_int),
        ("nodes_count", C.c_int), ("nodes", _dp), ("elements_count", C.c_int), ("elements", _ip),
        ("prescribed_nodes_count", C.c_int), ("presc_node", _ip), ("presc_type", _ip), ("presc_values", _dp),
        ("surface_faces_count", C.c_int), ("surface_nodes_per_face", C.c_int), ("surface_nodes", _ip),
        ("surface_kind", _ip), ("surface_values", _dp),
        ("materials_count", C.c_int), ("material_params", _dp), ("element_material", _ip),
        ("has_dynamics", C.c_int), ("dynamics_steps", C.c_int), ("dynamics_dt", C.c_double), ("dynamics_beta", C.c_double),
        ("dynamics_gamma", C.c_double), ("dynamics_dlambda", C.c_double), ("density", C.c_double),
        ("has_body_force", C.c_int), ("body_force", C.c_double * 3),
        ("dynamics_explicit", C.c_int), ("dynamics_safety", C.c_double), ("dynamics_restep", C.c_int),
        ("results_nodal_stress", C.c_int), ("results_energy", C.c_int), ("results_reactions", C.c_int),
        ("transient_sn_exponent", C.c_double), ("transient_sn_coefficient", C.c_double), ("transient_rainflow_depth", C.c_int),
        ("random_sn_exponent", C.c_double), ("random_sn_coefficient", C.c_double), ("random_duration", C.c_double),
        ("harmonic_stress", C.c_int), ("transient_stress", C.c_int),
        ("spectrum_stress", C.c_int), ("random_stress", C.c_int),
        ("has_spectrum", C.c_int), ("spectrum_count", C.c_int), ("spectrum_points", _dp), ("spectrum_rule", C.c_int),
        ("spectrum_static", C.c_int), ("spectrum_loglog", C.c_int), ("spectrum_has_base", C.c_int),
        ("spectrum_zeta", C.c_double), ("spectrum_zpa", C.c_double), ("spectrum_base", C.c_double * 3),
        ("has_random", C.c_int), ("random_count", C.c_int), ("random_points", _dp), ("random_static", C.c_int),
        ("random_loglog", C.c_int), ("random_per_mode", C.c_int), ("random_background", C.c_int), ("random_has_base", C.c_int),
        ("random_zeta", C.c_double), ("random_base", C.c_double * 3),
        ("transient_steps", C.c_int), ("transient_dt", C.c_double), ("transient_zeta", C.c_double),
        ("transient_static", C.c_int), ("transient_shape", C.c_int), ("transient_rise", C.c_double),
        ("transient_has_base", C.c_int), ("transient_base", C.c_double * 3),
        ("harmonic_count", C.c_int), ("harmonic_from", C.c_double), ("harmonic_to", C.c_double),
        ("harmonic_zeta", C.c_double), ("harmonic_static", C.c_int),
        ("damping_alpha", C.c_double), ("damping_beta", C.c_double),
        ("contact_faces_count", C.c_int), ("contact_nodes_per_face", C.c_int), ("contact_nodes", _ip),
        ("contact_obstacles_count", C.c_int), ("contact_kind", _ip), ("contact_geom", _dp),
        ("contact_penalty", C.c_double), ("contact_augment", C.c_int), ("contact_gap_tolerance", C.c_double),
        ("buckling_modes", C.c_int), ("buckling_tolerance", C.c_double), ("buckling_max", C.c_int),
        ("modal_count", C.c_int), ("modal_shift", C.c_double),
        ("modal_modes", C.c_int), ("modal_tolerance", C.c_double), ("modal_max", C.c_int),
    ]


class StepSnapshot(C.Structure):
    """struct fea_step_snapshot of host/fea_host.h."""
    _fields_ = [("nodes", _dp), ("stress0", _dp), ("nodal_stress", _dp), ("von_mises", _dp), ("contact_pressure", _dp)]


def export_gmsh(path, deck, nodes_steps, stress0_steps, nodal_stress_steps=None, von_mises_steps=None):
    """fea_export_gmsh: nodes_steps[k] is [N][3], stress0_steps[k] is [E][3][3] after load step k+1; with
    nodal_stress_steps[k] ([N][6]) and von_mises_steps[k] ([N]) every step also gets its two nodal-stress sections."""
    h = load_host_library()
    n = len(nodes_steps)
    keep = [(np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64))
            for a, b in zip(nodes_steps, stress0_steps)]
    nodal = [(np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64))
             for a, b in zip(nodal_stress_steps or [], von_mises_steps or [])]
    arr = (StepSnapshot * max(n, 1))()
    for k, (a, b) in enumerate(keep):
        arr[k].nodes, arr[k].stress0 = _d(a), _d(b)
    for k, (a, b) in enumerate(nodal[:n]):
        arr[k].nodal_stress, arr[k].von_mises = _d(a), _d(b)
    fd = deck.to_struct()
    if h.fea_export_gmsh(os.fsencode(path), C.byref(fd), arr, n) != 0:
        raise FeaHipError(f"could not write {path}")


def load_host_library():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise FeaHipError(f"{HOST_LIB_PATH} is missing: run __graft_entry__.build()")
        load_library()   # libfeahost.so links against libfeahip.so
        h = C.CDLL(HOST_LIB_PATH)
        h.fea_deck_load.argtypes = [C.c_char_p, C.POINTER(FeaDeck), C.c_char_p, C.c_int]
        h.fea_deck_load.restype = C.c_int
        h.fea_deck_free.argtypes = [C.POINTER(FeaDeck)]
        h.fea_deck_free.restype = None
        h.fea_deck_save.argtypes = [C.c_char_p, C.POINTER(FeaDeck)]
        h.fea_deck_save.restype = C.c_int
        h.fea_element_tables.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp]
        h.fea_element_tables.restype = C.c_int
        h.fea_deck_create_solver.argtypes = [C.POINTER(FeaDeck), C.c_int, C.POINTER(C.c_void_p), C.c_char_p, C.c_int]
        h.fea_deck_create_solver.restype = C.c_int
        h.fea_solve.argtypes = [C.POINTER(FeaDeck), C.c_void_p, C.c_void_p, _dp, C.c_int]
        h.fea_solve.restype = C.c_int
        h.fea_export_gmsh.argtypes = [C.c_char_p, C.POINTER(FeaDeck), C.POINTER(StepSnapshot), C.c_int]
        h.fea_export_gmsh.restype = C.c_int
        h.fea_export_name.argtypes = [C.c_char_p, C.c_char_p]
        h.fea_export_name.restype = None
        _host = h
    return _host


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def host_modal_ritz(gram_m, gram_k):
    """feahip_host_modal_ritz (no device): (rank kept, theta[8], coef[n_dirs][16]) of one Rayleigh-Ritz step."""
    lib = load_library()
    gm, gk = np.ascontiguousarray(gram_m, dtype=np.float64), np.ascontiguousarray(gram_k, dtype=np.float64)
    n = len(gm)
    assert gm.shape == (n, n) and gk.shape == (n, n)
    theta, coef = np.zeros(MODAL_COLS), np.zeros((n, 2 * MODAL_COLS))
    rank = lib.feahip_host_modal_ritz(n, _d(gm), _d(gk), _d(theta), _d(coef))
    return rank, theta, coef


def host_buckling_factor(nu):
    """feahip_host_buckling_factor (no device): 1 - 1/nu where nu < 0, +infinity elsewhere."""
    lib = load_library()
    nu = np.ascontiguousarray(np.atleast_1d(nu), dtype=np.float64)
    factor = np.zeros(len(nu))
    if lib.feahip_host_buckling_factor(len(nu), _d(nu), _d(factor)) != 0:
        raise FeaHipError("feahip_host_buckling_factor failed")
    return factor


def host_response_coefficients(lam, q, omega, alpha=0.0, beta=0.0, zeta=None, static_correction=True):
    """feahip_host_response_coefficients (no device): the complex table a[n_freq][64] of a sweep, a_k = q_k H_k or, with
    the correction, q_k (H_k - 1 / lam_k), H_k = 1 / (lam_k - w^2 + i w (alpha + beta lam_k + 2 zeta_k sqrt(lam_k))); zero
    past the modes given.  Raises where the sweep refuses (a negative input, a coefficient that is not finite)."""
    lam, q = np.ascontiguousarray(lam, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)
    omega = np.ascontiguousarray(np.atleast_1d(omega), dtype=np.float64)
    z = None if zeta is None else np.ascontiguousarray(zeta, dtype=np.float64)
    assert lam.shape == q.shape and lam.ndim == 1 and (z is None or z.shape == lam.shape)
    coef = np.zeros((len(omega), 2, MODAL_MAX_LOCKED))
    rc = load_library().feahip_host_response_coefficients(len(lam), _d(lam), _d(q), len(omega), _d(omega), float(alpha),
                                                          float(beta), None if z is None else _d(z), int(bool(static_correction)),
                                                          _d(coef))
    if rc != 0:
        raise FeaHipError(f"feahip_host_response_coefficients refused its input ({rc})")
    return coef[:, 0, :] + 1j * coef[:, 1, :]


def host_transient_coefficients(lam, q, g, dt, alpha=0.0, beta=0.0, zeta=None, static_correction=True, quantity=0):
    """feahip_host_transient_coefficients (no device): the table a[n_steps + 1][64] of a transient under q_k g(t), g given
    at t_n = n dt and linear in between, every mode advanced from rest by its exact propagator.  quantity 0: q_k(t_n), or
    with the correction q_k(t_n) - q_k g_n / lam_k; 1: q_k'(t_n); 2: q_k g_n - d_k q_k' - lam_k q_k.  Zero past the modes
    given.  Raises where the transient refuses."""
    lam, q = np.ascontiguousarray(lam, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)
    g = np.ascontiguousarray(np.atleast_1d(g), dtype=np.float64)
    z = None if zeta is None else np.ascontiguousarray(np.broadcast_to(np.asarray(zeta, dtype=np.float64), lam.shape))
    assert lam.shape == q.shape and lam.ndim == 1 and g.ndim == 1
    coef = np.zeros((max(len(g), 1), MODAL_MAX_LOCKED))
    rc = load_library().feahip_host_transient_coefficients(len(lam), _d(lam), _d(q), len(g) - 1, float(dt), _d(g), float(alpha),
                                                           float(beta), None if z is None else _d(z),
                                                           int(bool(static_correction)), int(quantity), _d(coef))
    if rc != 0:
        raise FeaHipError(f"feahip_host_transient_coefficients refused its input ({rc})")
    return coef


def host_harmonic_von_mises(sig6):
    """feahip_host_harmonic_von_mises (no device): the largest von Mises stress over the cycle of the harmonic stress
    state Re(sig6 exp(i w t)), sig6 complex [..., 6] as xx yy zz xy yz xz; vectorised over the leading axes."""
    lib = load_library()
    s = np.asarray(sig6, dtype=np.complex128)
    assert s.shape[-1] == 6
    flat = s.reshape(-1, 6)
    re, im = np.ascontiguousarray(flat.real), np.ascontiguousarray(flat.imag)
    out = np.zeros(len(flat))
    for k in range(len(flat)):
        out[k] = lib.feahip_host_harmonic_von_mises(_d(re[k]), _d(im[k]))
    return out.reshape(s.shape[:-1])


def _modal_arrays(lam, q, zeta):
    lam, q = np.ascontiguousarray(lam, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)
    z = None if zeta is None else np.ascontiguousarray(np.broadcast_to(np.asarray(zeta, dtype=np.float64), lam.shape))
    assert lam.shape == q.shape and lam.ndim == 1
    return lam, q, z


def host_random_form(lam, q, omega, S, alpha=0.0, beta=0.0, zeta=None, static_correction=True, quantity=0):
    """feahip_host_random_form (no device): (C[n][n], b[n], s) of the RMS under the one-sided PSD S(omega) per rad/s of the
    load factor, omega strictly ascending, trapezoid weights: C_kl = sum_j wt_j S_j w_j^(2p) Re(a_k conj(a_l)), b_k = sum_j
    wt_j S_j w_j^(2p) Re(a_k), s = sum_j wt_j S_j w_j^(2p), a the rows of host_response_coefficients, p = quantity.  b and s
    are zero without the correction.  Raises where the entry refuses."""
    lam, q, z = _modal_arrays(lam, q, zeta)
    omega, S = np.ascontiguousarray(omega, dtype=np.float64), np.ascontiguousarray(S, dtype=np.float64)
    assert omega.ndim == 1 and omega.shape == S.shape
    n = len(lam)
    Cm, b, s = np.zeros((n, n)), np.zeros(n), C.c_double(0)
    rc = load_library().feahip_host_random_form(n, _d(lam), _d(q), len(omega), _d(omega), _d(S), float(alpha), float(beta),
                                                None if z is None else _d(z), int(bool(static_correction)), int(quantity),
                                                _d(Cm), _d(b), C.byref(s))
    if rc != 0:
        raise FeaHipError(f"feahip_host_random_form refused its input ({rc})")
    return Cm, b, s.value


def host_moment_form(lam, q, omega, S, alpha=0.0, beta=0.0, zeta=None, static_correction=True, order=0):
    """feahip_host_moment_form (no device): (C[n][n], b[n], s) of the spectral moment m_order = integral of w^order G(w) dw of
    every linear combination of the response, order in (0, 1, 2, 4): host_random_form with the weight wt_j S_j w_j^order.  The
    orders 0, 2, 4 are that entry at quantity 0, 1, 2, bit for bit.  Raises where the entry refuses."""
    lam, q, z = _modal_arrays(lam, q, zeta)
    omega, S = np.ascontiguousarray(omega, dtype=np.float64), np.ascontiguousarray(S, dtype=np.float64)
    assert omega.ndim == 1 and omega.shape == S.shape
    n = len(lam)
    Cm, b, s = np.zeros((n, n)), np.zeros(n), C.c_double(0)
    rc = load_library().feahip_host_moment_form(n, _d(lam), _d(q), len(omega), _d(omega), _d(S), float(alpha), float(beta),
                                                None if z is None else _d(z), int(bool(static_correction)), int(order),
                                                _d(Cm), _d(b), C.byref(s))
    if rc != 0:
        raise FeaHipError(f"feahip_host_moment_form refused its input ({rc})")
    return Cm, b, s.value


FATIGUE_NO_STRESS, FATIGUE_NARROW, FATIGUE_NO_DIRLIK = 1, 2, 4      # the status bits of csrc/fatigue_point.h
FATIGUE_DAMAGE = ("narrow-band", "dirlik", "tovo-benasciutti")      # the last axis of a damage array


def host_fatigue(m, sn_exponent, sn_coefficient):
    """feahip_host_fatigue (no device): (rates[...][2], damage[...][3], status[...]) of the moments m[...][4] = (m0, m1, m2,
    m4) on the S-N curve N s^b = A (s the stress amplitude), in long double and rounded once: nu0 and nup in cycles per
    unit time, the damage per unit time by the narrow-band formula, Dirlik and Tovo-Benasciutti, the status bits
    FATIGUE_*.  Raises where the entry refuses (b outside [1, 64], A <= 0, a moment negative or not finite)."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    assert m.ndim >= 1 and m.shape[-1] == 4
    lead = m.shape[:-1]
    n = int(np.prod(lead, dtype=np.int64))
    rates, damage, status = np.zeros(lead + (2,)), np.zeros(lead + (3,)), np.zeros(lead, dtype=np.int32)
    rc = load_library().feahip_host_fatigue(n, _d(m), float(sn_exponent), float(sn_coefficient), _d(rates), _d(damage), _i(status))
    if rc != 0:
        raise FeaHipError(f"feahip_host_fatigue refused its input ({rc})")
    return rates, damage, status


RAINFLOW_MAX_DEPTH = 1024                               # FEA_RAINFLOW_MAX_DEPTH of include/fea_hip.h
RAINFLOW_MAX_PROJ = 48                                  # FEA_RAINFLOW_MAX_PROJ
RAINFLOW_CONSTANT, RAINFLOW_OVERFLOW = 1, 2             # the status bits of csrc/rainflow_point.h


def host_rainflow(series, sn_exponent, sn_coefficient, depth=32):
    """feahip_host_rainflow (no device): the rainflow count of one history by ASTM E1049-85's three-point rule on a ring of
    `depth` points, as a dict: damage (Miner's sum of count (range / 2)^b / A on the S-N curve N s^b = A, summed in long
    double and rounded once), cycles, max_range, depth_used, status (the bits RAINFLOW_*), and the counted cycles in
    counting order as ranges, means, counts.  Raises where the entry refuses (no sample, a sample that is not finite, b
    outside [1, 64], A <= 0, depth outside [4, RAINFLOW_MAX_DEPTH])."""
    x = np.ascontiguousarray(series, dtype=np.float64).reshape(-1)
    n = len(x)
    cap = max(n, 1)
    dmg, cyc, rng = C.c_double(0), C.c_double(0), C.c_double(0)
    used, status, counted = C.c_int(0), C.c_int(0), C.c_int(0)
    r, m, k = np.zeros(cap), np.zeros(cap), np.zeros(cap)
    rc = load_library().feahip_host_rainflow(n, _d(x), float(sn_exponent), float(sn_coefficient), int(depth), C.byref(dmg),
                                             C.byref(cyc), C.byref(rng), C.byref(used), C.byref(status), cap, C.byref(counted),
                                             _d(r), _d(m), _d(k))
    if rc != 0:
        raise FeaHipError(f"feahip_host_rainflow refused its input ({rc})")
    c = counted.value
    return dict(damage=dmg.value, cycles=cyc.value, max_range=rng.value, depth_used=used.value, status=status.value,
                ranges=r[:c].copy(), means=m[:c].copy(), counts=k[:c].copy())


def plane_projections(normals):
    """The rows [n][6] that project a stress state (xx, yy, zz, xy, yz, xz) onto the normal stress n' sigma n of the planes
    with the normals given: (nx^2, ny^2, nz^2, 2 nx ny, 2 ny nz, 2 nx nz) of the normalised normals -- the `projections`
    of FeaSolver.response_stress_rainflow."""
    nn = np.atleast_2d(np.asarray(normals, dtype=np.float64))
    assert nn.ndim == 2 and nn.shape[1] == 3
    length = np.sqrt((nn * nn).sum(axis=1))
    assert np.all(length > 0) and np.all(np.isfinite(length))
    u = nn / length[:, None]
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    return np.ascontiguousarray(np.stack([x * x, y * y, z * z, 2 * x * y, 2 * y * z, 2 * x * z], axis=1))


def host_random_grid(lam, alpha=0.0, beta=0.0, zeta=None, w_lo=0.0, w_hi=1.0, n_background=257, n_per_mode=64, breakpoints=()):
    """feahip_host_random_grid (no device): the sorted union, clipped to [w_lo, w_hi] and without duplicates, of n_background
    points of linspace(w_lo, w_hi), per mode with lam_k > 0 and d_k > 0 the n_per_mode points w_k + (d_k / 2) tan(theta_i),
    theta_i = ((i + 1/2) / n_per_mode) pi - pi / 2, and the breakpoints given."""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    z = None if zeta is None else np.ascontiguousarray(np.broadcast_to(np.asarray(zeta, dtype=np.float64), lam.shape))
    bp = np.ascontiguousarray(breakpoints, dtype=np.float64).reshape(-1)
    out = np.zeros(max(int(n_background), 0) + len(lam) * max(int(n_per_mode), 0) + len(bp) + 1)
    out[:len(bp)] = bp
    n = C.c_int(len(bp))
    rc = load_library().feahip_host_random_grid(len(lam), _d(lam), float(alpha), float(beta), None if z is None else _d(z),
                                                float(w_lo), float(w_hi), int(n_background), int(n_per_mode), _d(out), C.byref(n))
    if rc != 0:
        raise FeaHipError(f"feahip_host_random_grid refused its input ({rc})")
    return out[:n.value].copy()


def _table_value(fn, w, v, at, loglog):
    w, v = np.ascontiguousarray(w, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
    assert w.ndim == 1 and w.shape == v.shape
    out = np.array([fn(len(w), _d(w), _d(v), int(bool(loglog)), float(x)) for x in np.atleast_1d(at)])
    if np.isnan(out).any():
        raise FeaHipError("the table's points must be finite, their abscissae strictly ascending, and so the argument")
    return out if np.ndim(at) else float(out[0])


def host_psd_value(w, S, at, loglog=False):
    """feahip_host_psd_value (no device): the table (w, S) at `at` (a number or an array), linear or log-log, zero outside."""
    return _table_value(load_library().feahip_host_psd_value, w, S, at, loglog)


def host_spectrum_value(w, sa, at, loglog=False):
    """feahip_host_spectrum_value (no device): as host_psd_value, with the end values outside the table."""
    return _table_value(load_library().feahip_host_spectrum_value, w, sa, at, loglog)


def host_spectrum_form(lam, q, sa, rule=SRSS, alpha=0.0, beta=0.0, zeta=None, static_correction=False, zpa=0.0, quantity=0):
    """feahip_host_spectrum_form (no device): (C[n][n], b[n], s) of a response spectrum with the spectral accelerations
    sa[n] at the modes: a_k = q_k sa_k / lam_k (times sqrt(lam_k), lam_k for quantity 1, 2), SRSS C = diag(a^2), CQC C_jk =
    rho_jk a_j a_k (Der Kiureghian), ABS C = |a||a|'; with static_correction and zpa > 0 the missing mass, C += zpa^2 c c',
    b = zpa^2 c, s = zpa^2, c = -q / lam.  Raises where the entry refuses."""
    lam, q, z = _modal_arrays(lam, q, zeta)
    sa = np.ascontiguousarray(np.broadcast_to(np.asarray(sa, dtype=np.float64), lam.shape))
    n = len(lam)
    Cm, b, s = np.zeros((n, n)), np.zeros(n), C.c_double(0)
    rc = load_library().feahip_host_spectrum_form(n, _d(lam), _d(q), _d(sa), float(alpha), float(beta),
                                                  None if z is None else _d(z), int(rule), int(bool(static_correction)),
                                                  float(zpa), int(quantity), _d(Cm), _d(b), C.byref(s))
    if rc != 0:
        raise FeaHipError(f"feahip_host_spectrum_form refused its input ({rc})")
    return Cm, b, s.value


def host_rayleigh(omega1, zeta1, omega2, zeta2):
    """feahip_host_rayleigh (no device): (alpha, beta_k) of C = alpha M + beta_k K that give the damping ratios zeta1, zeta2
    at the circular frequencies omega1, omega2.  A negative coefficient is returned as it is (set_damping refuses it)."""
    a, b = C.c_double(0), C.c_double(0)
    rc = load_library().feahip_host_rayleigh(omega1, zeta1, omega2, zeta2, C.byref(a), C.byref(b))
    if rc != 0:
        raise FeaHipError(f"feahip_host_rayleigh: two different positive frequencies, please ({rc})")
    return a.value, b.value


def element_tables(ele_type, gauss_count):
    """(weights[G], forms[G][npe], dforms[G][3][npe]) from the host plug-in."""
    h = load_host_library()
    npe = {TETRAHEDRA10: 10, TETRAHEDRA4: 4, HEXAHEDRA8: 8}[ele_type]
    w = np.zeros(gauss_count)
    forms = np.zeros((gauss_count, npe))
    dforms = np.zeros((gauss_count, 3, npe))
    rc = h.fea_element_tables(ele_type, gauss_count, _d(w), _d(forms), _d(dforms))
    if rc < 0:
        raise FeaHipError(f"unsupported element type {ele_type} with {gauss_count} Gauss points")
    return w, forms, dforms


def _take_dynamics(obj, kw):
    """The implicit-dynamics fields of a Deck or a Slab: density (a number, or one per material for FeaSolver.set_mass; the
    .sexp grammar holds one number), body_force[3] (an acceleration per unit mass) and dynamics = dict(steps, dt, beta,
    gamma, dlambda) -- or, for the explicit scheme, dict(steps, dt, dlambda, scheme="explicit", safety, restep), where
    dt = 0 asks for safety times the stable-step estimate, made again every restep steps.  damping = (alpha, beta_k) of
    FeaSolver.set_damping, taken at the reference configuration when the solver is made."""
    dm = kw.get("damping")
    obj.damping = None if dm is None else (float(dm[0]), float(dm[1]))
    if obj.damping is not None and not all(0.0 <= v < np.inf for v in obj.damping):
        raise ValueError("damping: two finite coefficients that are not negative")
    obj.density = kw.get("density")
    bf = kw.get("body_force")
    obj.body_force = None if bf is None else np.ascontiguousarray(bf, dtype=np.float64).reshape(3)
    dyn = kw.get("dynamics")
    obj.dynamics = None if dyn is None else {"steps": int(dyn.get("steps", 0)), "dt": float(dyn["dt"]),
                                             "beta": float(dyn.get("beta", 0.25)), "gamma": float(dyn.get("gamma", 0.5)),
                                             "dlambda": float(dyn.get("dlambda", 0.0))}
    if dyn is not None and dyn.get("scheme", "newmark") != "newmark":
        if dyn["scheme"] != "explicit":
            raise ValueError("dynamics scheme: newmark or explicit")
        obj.dynamics.update(scheme="explicit", safety=float(dyn.get("safety", 0.9)), restep=int(dyn.get("restep", 0)))
    elif dyn is not None and ("safety" in dyn or "restep" in dyn):
        raise ValueError("safety and restep belong to the explicit scheme")
    if (obj.dynamics is not None or obj.body_force is not None) and obj.density is None:
        raise ValueError("dynamics and body_force need a density")


OBSTACLE_PLANE, OBSTACLE_SPHERE, OBSTACLE_SPHERE_INSIDE, OBSTACLE_CYLINDER, OBSTACLE_CYLINDER_INSIDE = 0, 1, 2, 3, 4
MAX_OBSTACLES = 8


def obstacle_arrays(obstacles):
    """(kind[n], geom[n][10]) of feahip_set_contact from a list of dicts (kind, point | center, normal | axis | direction,
    radius, travel) or tuples (kind, point, direction, radius, travel)."""
    kind, geom = [], []
    for ob in obstacles:
        if isinstance(ob, dict):
            point = ob.get("point", ob.get("center", (0.0, 0.0, 0.0)))
            direction = ob.get("normal", ob.get("axis", ob.get("direction", (0.0, 0.0, 0.0))))
            ob = (ob["kind"], point, direction, ob.get("radius", 0.0), ob.get("travel", (0.0, 0.0, 0.0)))
        k, point, direction, radius, travel = ob
        kind.append(int(k))
        geom.append([*np.asarray(point, dtype=np.float64), *np.asarray(direction, dtype=np.float64), float(radius),
                     *np.asarray(travel, dtype=np.float64)])
    return (np.ascontiguousarray(kind, dtype=np.int32),
            np.ascontiguousarray(geom, dtype=np.float64).reshape(len(kind), 10))


def _take_contact(self, kw):
    """The contact fields of a Deck or a Slab (feahip_set_contact): faces as surface_faces, obstacles as set_contact."""
    faces = np.asarray(kw.get("contact_faces", np.zeros((0, 0))), dtype=np.int32)
    self.contact_faces = np.ascontiguousarray(faces.reshape(len(faces), -1) if faces.size else np.zeros((0, 0), dtype=np.int32))
    self.contact_obstacles = list(kw.get("contact_obstacles", []))
    self.contact_penalty = float(kw.get("contact_penalty", 0.0))
    self.contact_augment = int(kw.get("contact_augment", 0))
    self.contact_gap_tolerance = float(kw.get("contact_gap_tolerance", 0.0))


class Deck:
    """A task deck as numpy arrays (fields named as the reference's structs)."""

    def __init__(self, **kw):
        self.model = kw.get("model", MODEL_COMPRESSIBLE_NEOHOOKEAN)
        self.parameters = np.array(kw.get("parameters", [100.0, 100.0]), dtype=np.float64)
        self.solver_type = kw.get("solver_type", CG)
        self.solver_tolerance = kw.get("solver_tolerance", 1e-14)
        self.solver_max_iter = kw.get("solver_max_iter", 20000)
        self.ele_type = kw.get("ele_type", TETRAHEDRA10)
        self.load_increments_count = kw.get("load_increments_count", 1)
        self.desired_tolerance = kw.get("desired_tolerance", 1e-8)
        self.max_newton_count = kw.get("max_newton_count", 20)
        self.modified_newton = kw.get("modified_newton", True)
        self.gauss_nodes_count = kw.get("gauss_nodes_count", 5)
        self.linesearch_max = kw.get("linesearch_max", 0)
        self.arclength_max = kw.get("arclength_max", 0)       # > 0 with surface loads: feasolver_hip follows the path
        self.nodes = np.ascontiguousarray(kw["nodes"], dtype=np.float64)
        self.elements = np.ascontiguousarray(kw["elements"], dtype=np.int32)
        self.nodes_per_element = self.elements.shape[1]
        self.presc_node = np.ascontiguousarray(kw.get("presc_node", []), dtype=np.int32)
        self.presc_type = np.ascontiguousarray(kw.get("presc_type", []), dtype=np.int32)
        self.presc_values = np.ascontiguousarray(kw.get("presc_values", np.zeros((0, 3))), dtype=np.float64).reshape(-1, 3)
        # surface loads (feahip_set_surface_loads): faces[F][nodes per face] in any node order, kind[F] LOAD_*,
        # values[F][3] (pressure in [0], or the dead traction t0), per load increment
        faces = np.asarray(kw.get("surface_faces", np.zeros((0, 0))), dtype=np.int32)
        self.surface_faces = np.ascontiguousarray(faces.reshape(len(faces), -1) if faces.size else np.zeros((0, 0), dtype=np.int32))
        self.surface_kind = np.ascontiguousarray(kw.get("surface_kind", []), dtype=np.int32)
        self.surface_values = np.ascontiguousarray(kw.get("surface_values", np.zeros((0, 3))), dtype=np.float64).reshape(-1, 3)
        _take_contact(self, kw)
        # material table (feahip_set_materials): materials[n][2] = lambda, mu and one id per element; none = the single
        # pair `parameters`
        self.materials = np.ascontiguousarray(kw.get("materials", np.zeros((0, 2))), dtype=np.float64).reshape(-1, 2)
        self.element_material = np.ascontiguousarray(kw.get("element_material", []), dtype=np.int32)
        if len(self.element_material) != (len(self.elements) if len(self.materials) else 0):
            raise ValueError("materials and element_material come together, one id per element")
        _take_dynamics(self, kw)
        # (results :nodal-stress t :energy t :reactions t): what feasolver_hip adds to its .msh file and its log
        res = kw.get("results") or {}
        if set(res) - {"nodal_stress", "energy", "reactions"}:
            raise ValueError("results: nodal_stress, energy, reactions")
        self.results = {k: bool(res.get(k, False)) for k in ("nodal_stress", "energy", "reactions")}
        # (modal :modes N :tolerance t :max M): the natural frequencies feasolver_hip computes after its last step
        self.modal_modes = int(kw.get("modal_modes", 0))
        self.modal_tolerance = float(kw.get("modal_tolerance", 1e-8))
        self.modal_max = int(kw.get("modal_max", 1000))
        if not 0 <= self.modal_modes <= MODAL_COLS:
            raise ValueError("modal_modes: 0 to 8")
        # :count N (up to 64 modes, instead of :modes) and :shift s: the locked solve (solve_modes_locked)
        self.modal_count = int(kw.get("modal_count", 0))
        self.modal_shift = float(kw.get("modal_shift", 0.0))
        if not 0 <= self.modal_count <= MODAL_MAX_LOCKED:
            raise ValueError("modal_count: 1 to 64")
        if self.modal_count and self.modal_modes:
            raise ValueError("modal_modes or modal_count, not both")
        if not (0.0 <= self.modal_shift < np.inf):
            raise ValueError("modal_shift: finite and not negative")
        if self.modal_shift and not (self.modal_modes or self.modal_count):
            raise ValueError("modal_shift needs modal_modes or modal_count")
        if (self.modal_modes or self.modal_count) and self.density is None:
            raise ValueError("modal_modes needs a density")
        # (harmonic :from f0 :to f1 :count n :zeta z :static-correction t): the frequency sweep feasolver_hip makes on the
        # locked modes after the modal run, n linearly spaced frequencies in Hz under the surface load of the state reached
        self.harmonic_count = int(kw.get("harmonic_count", 0))
        self.harmonic_from = float(kw.get("harmonic_from", 0.0))
        self.harmonic_to = float(kw.get("harmonic_to", 0.0))
        self.harmonic_zeta = float(kw.get("harmonic_zeta", 0.0))
        self.harmonic_static = bool(kw.get("harmonic_static", True))
        self.harmonic_stress = bool(kw.get("harmonic_stress", False))          # :stress t: the peak von Mises stress as well
        if self.harmonic_stress and not self.harmonic_count:
            raise ValueError("harmonic_stress needs harmonic_count")
        if not 0 <= self.harmonic_count <= RESPONSE_MAX_FREQ:
            raise ValueError("harmonic_count: 1 to 4096")
        if self.harmonic_count:
            if not (0.0 <= self.harmonic_from <= self.harmonic_to < np.inf):
                raise ValueError("harmonic_from and harmonic_to: 0 <= from <= to, finite")
            if not (0.0 <= self.harmonic_zeta < np.inf):
                raise ValueError("harmonic_zeta: finite and not negative")
            if not (self.modal_count or self.modal_shift):
                raise ValueError("harmonic_count needs the locked modes: modal_count or modal_shift")
            if self.harmonic_static and self.modal_shift:
                raise ValueError("harmonic_static (the static correction) and a non-zero modal_shift exclude each other")
        # (transient :steps n :dt x :shape step|ramp|half-sine :rise T :zeta z :static-correction t :base (bx by bz)): the
        # time history feasolver_hip runs on the locked modes after the harmonic sweep, under the surface load of the state
        # reached or, with a base direction, under the base load
        self.transient_steps = int(kw.get("transient_steps", 0))
        self.transient_dt = float(kw.get("transient_dt", 0.0))
        self.transient_zeta = float(kw.get("transient_zeta", 0.0))
        self.transient_static = bool(kw.get("transient_static", True))
        self.transient_shape = kw.get("transient_shape", "step")
        self.transient_rise = float(kw.get("transient_rise", 0.0))
        base = kw.get("transient_base")
        self.transient_base = None if base is None else tuple(float(b) for b in base)
        self.transient_stress = bool(kw.get("transient_stress", False))        # :stress t: the peak von Mises stress as well
        if self.transient_stress and not self.transient_steps:
            raise ValueError("transient_stress needs transient_steps")
        # :sn-exponent b :sn-coefficient A :rainflow-depth d inside (transient ... :stress t): the rainflow count on N s^b = A
        self.transient_sn_exponent = float(kw.get("transient_sn_exponent", 0.0))
        self.transient_sn_coefficient = float(kw.get("transient_sn_coefficient", 0.0))
        self.transient_rainflow_depth = int(kw.get("transient_rainflow_depth", 32))
        if self.transient_sn_exponent:
            if not self.transient_stress:
                raise ValueError("transient_sn_exponent needs transient_stress")
            if not (1.0 <= self.transient_sn_exponent <= 64.0 and 0.0 < self.transient_sn_coefficient < np.inf
                    and 4 <= self.transient_rainflow_depth <= 1024):
                raise ValueError("transient_sn_exponent: 1 to 64, transient_sn_coefficient: positive and finite, transient_rainflow_depth: 4 to 1024")
        elif self.transient_sn_coefficient or self.transient_rainflow_depth != 32:
            raise ValueError("transient_sn_coefficient and transient_rainflow_depth need transient_sn_exponent")
        if not 0 <= self.transient_steps <= TRANSIENT_MAX_STEPS:
            raise ValueError("transient_steps: 1 to 1048576")
        if self.transient_steps:
            if not (0.0 < self.transient_dt < np.inf):
                raise ValueError("transient_dt: positive and finite")
            if not (0.0 <= self.transient_zeta < np.inf):
                raise ValueError("transient_zeta: finite and not negative")
            if self.transient_shape not in TRANSIENT_SHAPES:
                raise ValueError("transient_shape: step, ramp or half-sine")
            if self.transient_shape != "step" and not (0.0 < self.transient_rise < np.inf):
                raise ValueError("transient_rise: positive and finite for a ramp or a half-sine")
            if self.transient_base is not None and (len(self.transient_base) != 3 or not np.all(np.isfinite(self.transient_base))
                                                    or not any(self.transient_base)):
                raise ValueError("transient_base: three finite components, not all zero")
            if not (self.modal_count or self.modal_shift):
                raise ValueError("transient_steps needs the locked modes: modal_count or modal_shift")
            if self.transient_static and self.modal_shift:
                raise ValueError("transient_static (the static correction) and a non-zero modal_shift exclude each other")
        # (spectrum :base (bx by bz) :rule srss|cqc|abs :zeta z :static-correction t :zpa a :interp linear|loglog (points (f sa)
        # ...)) and (random :base (bx by bz) :zeta z :static-correction t :interp linear|loglog :per-mode n :background n (psd
        # (f s) ...)): the design peak under a response spectrum and the RMS under a PSD that feasolver_hip computes on the
        # locked modes after the transient run; f in Hz, s per Hz
        for name, floor in (("spectrum", 1), ("random", 2)):
            pts = kw.get(f"{name}_points")
            pts = np.zeros((0, 2)) if pts is None else np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
            setattr(self, f"{name}_points", pts)
            setattr(self, f"{name}_zeta", float(kw.get(f"{name}_zeta", 0.0)))
            setattr(self, f"{name}_static", bool(kw.get(f"{name}_static", True)))
            setattr(self, f"{name}_interp", kw.get(f"{name}_interp", "linear"))
            base = kw.get(f"{name}_base")
            base = None if base is None else tuple(float(b) for b in base)
            setattr(self, f"{name}_base", base)
            setattr(self, f"{name}_stress", bool(kw.get(f"{name}_stress", False)))     # :stress t: the von Mises result as well
            if not len(pts):
                if getattr(self, f"{name}_stress"):
                    raise ValueError(f"{name}_stress needs {name}_points")
                continue
            if not floor <= len(pts) <= DECK_MAX_POINTS:
                raise ValueError(f"{name}_points: {floor} to {DECK_MAX_POINTS} pairs")
            if not (np.all(np.isfinite(pts)) and np.all(pts >= 0) and np.all(np.diff(pts[:, 0]) > 0)):
                raise ValueError(f"{name}_points: finite and not negative, the frequencies strictly ascending")
            if not (0.0 <= getattr(self, f"{name}_zeta") < np.inf):
                raise ValueError(f"{name}_zeta: finite and not negative")
            if getattr(self, f"{name}_interp") not in ("linear", "loglog"):
                raise ValueError(f"{name}_interp: linear or loglog")
            if base is not None and (len(base) != 3 or not np.all(np.isfinite(base)) or not any(base)):
                raise ValueError(f"{name}_base: three finite components, not all zero")
            if not (self.modal_count or self.modal_shift):
                raise ValueError(f"{name}_points needs the locked modes: modal_count or modal_shift")
            if getattr(self, f"{name}_static") and self.modal_shift:
                raise ValueError(f"{name}_static (the static correction) and a non-zero modal_shift exclude each other")
        self.spectrum_rule = kw.get("spectrum_rule", "srss")
        self.spectrum_zpa = float(kw.get("spectrum_zpa", 0.0))
        self.random_per_mode = int(kw.get("random_per_mode", 32))
        self.random_background = int(kw.get("random_background", 257))
        if len(self.spectrum_points):
            if self.spectrum_rule not in SPECTRUM_RULES:
                raise ValueError("spectrum_rule: srss, cqc or abs")
            if not (0.0 <= self.spectrum_zpa < np.inf):
                raise ValueError("spectrum_zpa: finite and not negative")
            if self.spectrum_zpa and (not self.spectrum_static or self.spectrum_rule == "abs"):
                raise ValueError("spectrum_zpa needs spectrum_static and a rule other than abs")
            if self.spectrum_stress and self.spectrum_rule == "abs":
                raise ValueError("spectrum_stress needs a rule other than abs")
        # :sn-exponent b :sn-coefficient A :duration T inside (random ...): fatigue of the von Mises process on N s^b = A over T
        self.random_sn_exponent = float(kw.get("random_sn_exponent", 0.0))
        self.random_sn_coefficient = float(kw.get("random_sn_coefficient", 0.0))
        self.random_duration = float(kw.get("random_duration", 1.0))
        if self.random_sn_exponent:
            if not len(self.random_points):
                raise ValueError("random_sn_exponent needs random_points")
            if not (1.0 <= self.random_sn_exponent <= 64.0 and 0.0 < self.random_sn_coefficient < np.inf and 0.0 < self.random_duration < np.inf):
                raise ValueError("random_sn_exponent: 1 to 64, random_sn_coefficient and random_duration: positive and finite")
        elif self.random_sn_coefficient or self.random_duration != 1.0:
            raise ValueError("random_sn_coefficient and random_duration need random_sn_exponent")
        if len(self.random_points) and not (0 <= self.random_per_mode <= 4096 and 2 <= self.random_background <= 131072):
            raise ValueError("random_per_mode: 0 to 4096, random_background: 2 to 131072")
        # (buckling :modes N :tolerance t :max M): the load factors feasolver_hip computes after its last step
        self.buckling_modes = int(kw.get("buckling_modes", 0))
        self.buckling_tolerance = float(kw.get("buckling_tolerance", 1e-8))
        self.buckling_max = int(kw.get("buckling_max", 2000))
        if not 0 <= self.buckling_modes <= MODAL_COLS:
            raise ValueError("buckling_modes: 0 to 8")
        if not self.buckling_tolerance > 0:
            raise ValueError("buckling_tolerance: positive")
        if self.buckling_max < 0:
            raise ValueError("buckling_max: not negative")

    @staticmethod
    def load(path):
        """Reads a .sexp deck through the product's C reader."""
        h = load_host_library()
        fd = FeaDeck()
        err = C.create_string_buffer(512)
        if h.fea_deck_load(os.fsencode(path), C.byref(fd), err, 512) != 0:
            raise FeaHipError(f"{path}: {err.value.decode()}")
        try:
            n, e, npe, nb = fd.nodes_count, fd.elements_count, fd.nodes_per_element, fd.prescribed_nodes_count
            ns, npf, nm = fd.surface_faces_count, fd.surface_nodes_per_face, fd.materials_count
            nc, ncf, no = fd.contact_faces_count, fd.contact_nodes_per_face, fd.contact_obstacles_count
            ck = np.ctypeslib.as_array(fd.contact_kind, (no,)).copy() if no else []
            cg = np.ctypeslib.as_array(fd.contact_geom, (no, 10)).copy() if no else []
            deck = Deck(
                model=fd.model, parameters=[fd.parameters[0], fd.parameters[1]], solver_type=fd.solver_type,
                solver_tolerance=fd.solver_tolerance, solver_max_iter=fd.solver_max_iter, ele_type=fd.ele_type,
                load_increments_count=fd.load_increments_count, desired_tolerance=fd.desired_tolerance,
                max_newton_count=fd.max_newton_count, modified_newton=bool(fd.modified_newton),
                gauss_nodes_count=fd.gauss_nodes_count,
                nodes=np.ctypeslib.as_array(fd.nodes, (n, 3)).copy(),
                elements=np.ctypeslib.as_array(fd.elements, (e, npe)).copy(),
                presc_node=np.ctypeslib.as_array(fd.presc_node, (nb,)).copy() if nb else [],
                presc_type=np.ctypeslib.as_array(fd.presc_type, (nb,)).copy() if nb else [],
                presc_values=np.ctypeslib.as_array(fd.presc_values, (nb, 3)).copy() if nb else np.zeros((0, 3)),
                surface_faces=np.ctypeslib.as_array(fd.surface_nodes, (ns, npf)).copy() if ns else np.zeros((0, 0)),
                surface_kind=np.ctypeslib.as_array(fd.surface_kind, (ns,)).copy() if ns else [],
                surface_values=np.ctypeslib.as_array(fd.surface_values, (ns, 3)).copy() if ns else np.zeros((0, 3)),
                materials=np.ctypeslib.as_array(fd.material_params, (nm, 2)).copy() if nm else np.zeros((0, 2)),
                element_material=np.ctypeslib.as_array(fd.element_material, (e,)).copy() if nm else [],
                density=fd.density if fd.has_dynamics else None,
                body_force=[fd.body_force[k] for k in range(3)] if fd.has_body_force else None,
                dynamics=dict(steps=fd.dynamics_steps, dt=fd.dynamics_dt, beta=fd.dynamics_beta, gamma=fd.dynamics_gamma,
                              dlambda=fd.dynamics_dlambda,
                              **(dict(scheme="explicit", safety=fd.dynamics_safety, restep=fd.dynamics_restep)
                                 if fd.dynamics_explicit else {})) if fd.has_dynamics else None,
                damping=(fd.damping_alpha, fd.damping_beta) if fd.has_dynamics and (fd.damping_alpha or fd.damping_beta) else None,
                results=dict(nodal_stress=bool(fd.results_nodal_stress), energy=bool(fd.results_energy),
                             reactions=bool(fd.results_reactions)),
                **(dict(contact_faces=np.ctypeslib.as_array(fd.contact_nodes, (nc, ncf)).copy(),
                        contact_obstacles=[(int(k), g[0:3], g[3:6], float(g[6]), g[7:10]) for k, g in zip(ck, cg)],
                        contact_penalty=fd.contact_penalty, contact_augment=fd.contact_augment,
                        contact_gap_tolerance=fd.contact_gap_tolerance) if nc and no else {}),
                **(dict(modal_modes=fd.modal_modes, modal_count=fd.modal_count, modal_shift=fd.modal_shift,
                        modal_tolerance=fd.modal_tolerance, modal_max=fd.modal_max)
                   if fd.modal_modes or fd.modal_count else {}),
                **(dict(harmonic_count=fd.harmonic_count, harmonic_from=fd.harmonic_from, harmonic_to=fd.harmonic_to,
                        harmonic_zeta=fd.harmonic_zeta, harmonic_static=bool(fd.harmonic_static),
                        harmonic_stress=bool(fd.harmonic_stress))
                   if fd.harmonic_count else {}),
                **(dict(transient_steps=fd.transient_steps, transient_dt=fd.transient_dt, transient_zeta=fd.transient_zeta,
                        transient_static=bool(fd.transient_static), transient_shape=TRANSIENT_SHAPES[fd.transient_shape],
                        transient_rise=fd.transient_rise,
                        transient_base=[fd.transient_base[k] for k in range(3)] if fd.transient_has_base else None,
                        transient_stress=bool(fd.transient_stress),
                        **(dict(transient_sn_exponent=fd.transient_sn_exponent, transient_sn_coefficient=fd.transient_sn_coefficient,
                                transient_rainflow_depth=fd.transient_rainflow_depth) if fd.transient_sn_exponent else {}))
                   if fd.transient_steps else {}),
                **(dict(spectrum_points=np.ctypeslib.as_array(fd.spectrum_points, (fd.spectrum_count, 2)).copy(),
                        spectrum_rule=SPECTRUM_RULES[fd.spectrum_rule], spectrum_zeta=fd.spectrum_zeta, spectrum_zpa=fd.spectrum_zpa,
                        spectrum_static=bool(fd.spectrum_static), spectrum_interp="loglog" if fd.spectrum_loglog else "linear",
                        spectrum_base=[fd.spectrum_base[k] for k in range(3)] if fd.spectrum_has_base else None,
                        spectrum_stress=bool(fd.spectrum_stress))
                   if fd.has_spectrum else {}),
                **(dict(random_points=np.ctypeslib.as_array(fd.random_points, (fd.random_count, 2)).copy(),
                        random_zeta=fd.random_zeta, random_static=bool(fd.random_static),
                        random_interp="loglog" if fd.random_loglog else "linear", random_per_mode=fd.random_per_mode,
                        random_background=fd.random_background,
                        random_base=[fd.random_base[k] for k in range(3)] if fd.random_has_base else None,
                        random_stress=bool(fd.random_stress),
                        **(dict(random_sn_exponent=fd.random_sn_exponent, random_sn_coefficient=fd.random_sn_coefficient,
                                random_duration=fd.random_duration) if fd.random_sn_exponent else {}))
                   if fd.has_random else {}),
                **(dict(buckling_modes=fd.buckling_modes, buckling_tolerance=fd.buckling_tolerance,
                        buckling_max=fd.buckling_max) if fd.buckling_modes else {}))
            deck.linesearch_max, deck.arclength_max = fd.linesearch_max, fd.arclength_max
            return deck
        finally:
            h.fea_deck_free(C.byref(fd))

    def to_struct(self):
        fd = FeaDeck()
        fd.model = self.model
        fd.parameters[0], fd.parameters[1] = float(self.parameters[0]), float(self.parameters[1])
        fd.parameters_count = 2
        fd.solver_type, fd.solver_tolerance, fd.solver_max_iter = self.solver_type, self.solver_tolerance, self.solver_max_iter
        fd.ele_type = self.ele_type
        fd.load_increments_count, fd.desired_tolerance = self.load_increments_count, self.desired_tolerance
        fd.max_newton_count, fd.modified_newton = self.max_newton_count, int(self.modified_newton)
        fd.nodes_per_element, fd.gauss_nodes_count = self.nodes_per_element, self.gauss_nodes_count
        fd.linesearch_max, fd.arclength_max = int(self.linesearch_max), int(self.arclength_max)
        fd.nodes_count, fd.nodes = len(self.nodes), _d(self.nodes)
        fd.elements_count, fd.elements = len(self.elements), _i(self.elements)
        fd.prescribed_nodes_count = len(self.presc_node)
        fd.presc_node, fd.presc_type, fd.presc_values = _i(self.presc_node), _i(self.presc_type), _d(self.presc_values)
        fd.surface_faces_count = len(self.surface_kind)
        fd.surface_nodes_per_face = self.surface_faces.shape[1] if len(self.surface_kind) else 0
        fd.surface_nodes, fd.surface_kind, fd.surface_values = _i(self.surface_faces), _i(self.surface_kind), _d(self.surface_values)
        # (the arrays are the deck's own, contiguous and of the struct's types: the struct borrows them)
        self.materials = np.ascontiguousarray(self.materials, dtype=np.float64).reshape(-1, 2)
        self.element_material = np.ascontiguousarray(self.element_material, dtype=np.int32)
        fd.materials_count = len(self.materials)
        fd.material_params, fd.element_material = _d(self.materials), _i(self.element_material)
        if getattr(self, "density", None) is not None:
            rho = np.atleast_1d(np.asarray(self.density, dtype=np.float64))
            if len(rho) != 1:
                raise ValueError("the deck grammar holds one density; per-material densities go through set_mass")
            dyn = getattr(self, "dynamics", None) or {"steps": 0, "dt": 1.0, "beta": 0.25, "gamma": 0.5, "dlambda": 0.0}
            fd.has_dynamics, fd.density = 1, float(rho[0])
            fd.dynamics_steps, fd.dynamics_dt = dyn["steps"], dyn["dt"]
            fd.dynamics_beta, fd.dynamics_gamma, fd.dynamics_dlambda = dyn["beta"], dyn["gamma"], dyn["dlambda"]
            if dyn.get("scheme") == "explicit":
                fd.dynamics_explicit, fd.dynamics_safety, fd.dynamics_restep = 1, dyn["safety"], dyn["restep"]
            if getattr(self, "damping", None) is not None:
                fd.damping_alpha, fd.damping_beta = self.damping
            if getattr(self, "body_force", None) is not None:
                fd.has_body_force = 1
                for k in range(3):
                    fd.body_force[k] = float(self.body_force[k])
        elif getattr(self, "damping", None) is not None and any(self.damping):
            raise ValueError("the deck grammar holds the damping inside (dynamics ...): it needs a density")
        res = getattr(self, "results", None) or {}
        fd.results_nodal_stress, fd.results_energy = int(res.get("nodal_stress", False)), int(res.get("energy", False))
        fd.results_reactions = int(res.get("reactions", False))
        fd.modal_modes = int(getattr(self, "modal_modes", 0))
        fd.modal_count, fd.modal_shift = int(getattr(self, "modal_count", 0)), float(getattr(self, "modal_shift", 0.0))
        fd.modal_tolerance, fd.modal_max = float(getattr(self, "modal_tolerance", 1e-8)), int(getattr(self, "modal_max", 1000))
        if getattr(self, "harmonic_count", 0):
            fd.harmonic_count, fd.harmonic_from, fd.harmonic_to = int(self.harmonic_count), float(self.harmonic_from), float(self.harmonic_to)
            fd.harmonic_zeta, fd.harmonic_static = float(self.harmonic_zeta), int(bool(self.harmonic_static))
            fd.harmonic_stress = int(bool(getattr(self, "harmonic_stress", False)))
        if getattr(self, "transient_steps", 0):
            fd.transient_steps, fd.transient_dt, fd.transient_zeta = int(self.transient_steps), float(self.transient_dt), float(self.transient_zeta)
            fd.transient_static, fd.transient_shape = int(bool(self.transient_static)), TRANSIENT_SHAPES.index(self.transient_shape)
            fd.transient_rise = float(self.transient_rise)
            fd.transient_stress = int(bool(getattr(self, "transient_stress", False)))
            if getattr(self, "transient_sn_exponent", 0.0):
                fd.transient_sn_exponent, fd.transient_sn_coefficient = self.transient_sn_exponent, self.transient_sn_coefficient
                fd.transient_rainflow_depth = self.transient_rainflow_depth
            if self.transient_base is not None:
                fd.transient_has_base = 1
                for k in range(3):
                    fd.transient_base[k] = self.transient_base[k]
        if len(getattr(self, "spectrum_points", ())):                   # (the struct borrows the arrays of points)
            fd.has_spectrum, fd.spectrum_count, fd.spectrum_points = 1, len(self.spectrum_points), _d(self.spectrum_points)
            fd.spectrum_rule, fd.spectrum_static = SPECTRUM_RULES.index(self.spectrum_rule), int(bool(self.spectrum_static))
            fd.spectrum_loglog, fd.spectrum_zeta, fd.spectrum_zpa = int(self.spectrum_interp == "loglog"), self.spectrum_zeta, self.spectrum_zpa
            fd.spectrum_stress = int(bool(getattr(self, "spectrum_stress", False)))
            if self.spectrum_base is not None:
                fd.spectrum_has_base = 1
                for k in range(3):
                    fd.spectrum_base[k] = self.spectrum_base[k]
        if len(getattr(self, "random_points", ())):
            fd.has_random, fd.random_count, fd.random_points = 1, len(self.random_points), _d(self.random_points)
            fd.random_static, fd.random_loglog, fd.random_zeta = int(bool(self.random_static)), int(self.random_interp == "loglog"), self.random_zeta
            fd.random_per_mode, fd.random_background = int(self.random_per_mode), int(self.random_background)
            fd.random_stress = int(bool(getattr(self, "random_stress", False)))
            if getattr(self, "random_sn_exponent", 0.0):
                fd.random_sn_exponent, fd.random_sn_coefficient = self.random_sn_exponent, self.random_sn_coefficient
                fd.random_duration = self.random_duration
            if self.random_base is not None:
                fd.random_has_base = 1
                for k in range(3):
                    fd.random_base[k] = self.random_base[k]
        if len(self.contact_faces) and len(self.contact_obstacles):
            # (kept on the deck: the struct borrows the arrays)
            self._contact_kind, self._contact_geom = obstacle_arrays(self.contact_obstacles)
            fd.contact_faces_count, fd.contact_nodes_per_face = self.contact_faces.shape
            fd.contact_nodes, fd.contact_obstacles_count = _i(self.contact_faces), len(self._contact_kind)
            fd.contact_kind, fd.contact_geom = _i(self._contact_kind), _d(self._contact_geom)
            fd.contact_penalty, fd.contact_augment = self.contact_penalty, self.contact_augment
            fd.contact_gap_tolerance = self.contact_gap_tolerance
        fd.buckling_modes = int(getattr(self, "buckling_modes", 0))
        fd.buckling_tolerance = float(getattr(self, "buckling_tolerance", 1e-8))
        fd.buckling_max = int(getattr(self, "buckling_max", 2000))
        return fd

    def save(self, path):
        h = load_host_library()
        fd = self.to_struct()
        if h.fea_deck_save(os.fsencode(path), C.byref(fd)) != 0:
            raise FeaHipError(f"could not write {path}")


class FeaSolver:
    """The `fea_solver` object of the reference, backed by the HIP context.

    Method names are the reference's solver_* functions minus the prefix
    (fea_solver.h:497-610)."""

    def __init__(self, deck, device=0):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        self.deck = deck
        w, _, dforms = element_tables(deck.ele_type, deck.gauss_nodes_count)
        self.N, self.E = len(deck.nodes), len(deck.elements)
        self.npe, self.G = deck.nodes_per_element, deck.gauss_nodes_count
        self.ndof = 3 * self.N
        par = np.zeros(10)
        par[:2] = deck.parameters[:2]
        rc = self._lib.feahip_create(
            C.byref(self._ctx), device, self.N, self.E, self.npe, self.G, _d(w), _d(dforms), _i(deck.elements),
            _d(deck.nodes), deck.model, _d(par), 2, len(deck.presc_node), _i(deck.presc_node), _i(deck.presc_type),
            _d(deck.presc_values))
        if rc != 0:
            self._ctx = C.c_void_p()
            raise FeaHipError(f"feahip_create failed ({rc}): {self._lib.feahip_create_error().decode()}")
        self._deck_surface_loads()
        self._deck_contact()
        self._deck_materials()
        self._deck_mass()

    def _deck_mass(self):
        """Installs the deck's (or the slab's) density, body force and damping, where it has them."""
        if getattr(self.deck, "density", None) is not None:
            self.set_mass(self.deck.density)
            if getattr(self.deck, "body_force", None) is not None:
                self.set_body_force(self.deck.body_force)
        if getattr(self.deck, "damping", None) is not None and any(self.deck.damping):
            self.set_damping(*self.deck.damping)

    def _deck_materials(self):
        """Installs the deck's (or the slab's) material table, where it has one."""
        if len(getattr(self.deck, "materials", [])):
            self.set_materials(self.deck.materials, self.deck.element_material)

    def set_materials(self, materials, element_material=None):
        """feahip_set_materials: materials[n][2] = (lambda, mu), element_material[E] in [0, n) in the order of the
        elements this solver was made from (the whole deck's for a RankSolver, the slab's for a LocalRankSolver).
        set_materials(None) (or an empty table) returns to the single pair of the deck."""
        par = np.ascontiguousarray(np.zeros((0, 2)) if materials is None else materials, dtype=np.float64).reshape(-1, 2)
        ids = np.ascontiguousarray([] if element_material is None else element_material, dtype=np.int32).ravel()
        n = len(par)
        ne = len(self.deck.elements)
        if n and len(ids) != ne:
            raise ValueError(f"element_material has {len(ids)} entries for {ne} elements")
        self._chk(self._lib.feahip_set_materials(self._ctx, n, _d(par) if n else None, _i(ids) if n else None))

    def materials(self):
        """(materials[n][2], element_material[this context's elements]) in force; ([0][2], []) without a table."""
        n = C.c_int(0)
        self._chk(self._lib.feahip_get_materials(self._ctx, C.byref(n), None, None))
        par, ids = np.zeros((n.value, 2)), np.zeros(self.E if n.value else 0, dtype=np.int32)
        if n.value:
            self._chk(self._lib.feahip_get_materials(self._ctx, C.byref(n), _d(par), _i(ids)))
        return par, ids

    def _deck_surface_loads(self):
        if len(getattr(self.deck, "surface_kind", [])):
            d = self.deck
            self.set_surface_loads(d.surface_faces, d.surface_kind, d.surface_values)

    def _deck_contact(self):
        d = self.deck
        if len(getattr(d, "contact_obstacles", [])) and (len(d.contact_faces) or isinstance(d, Slab)):
            # (a slab without a contact face of its own still takes the obstacles: its rank joins the collectives)
            self.set_contact(d.contact_faces, d.contact_obstacles, d.contact_penalty, d.contact_augment, d.contact_gap_tolerance)

    def close(self):
        if self._ctx:
            self._lib.feahip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise FeaHipError(f"libfeahip error {rc}: {self._lib.feahip_last_error(self._ctx).decode()}")

    # ---- the calls of solve() ------------------------------------------
    def update_nodes_with_bc(self, lam):
        self._chk(self._lib.feahip_update_nodes_with_bc(self._ctx, lam))

    def update_state(self):
        bad = C.c_int(0)
        self._chk(self._lib.feahip_update_state(self._ctx, C.byref(bad)))
        return bad.value

    def create_stiffness(self):
        self._chk(self._lib.feahip_create_stiffness(self._ctx))

    def create_residual_forces(self):
        self._chk(self._lib.feahip_create_residual_forces(self._ctx))

    def create_stiffness_and_residual(self):
        self._chk(self._lib.feahip_create_stiffness_and_residual(self._ctx))

    def stash_stiffness(self):
        self._chk(self._lib.feahip_stash_stiffness(self._ctx))

    def restore_stiffness(self):
        self._chk(self._lib.feahip_restore_stiffness(self._ctx))

    def apply_prescribed_bc(self, lam):
        self._chk(self._lib.feahip_apply_prescribed_bc(self._ctx, lam))

    def solve_slae(self, solver_type=None, tolerance=None, max_iterations=None):
        it, res = C.c_int(0), C.c_double(0)
        d = self.deck
        self._chk(self._lib.feahip_solve_slae(
            self._ctx, d.solver_type if solver_type is None else solver_type,
            d.solver_tolerance if tolerance is None else tolerance,
            d.solver_max_iter if max_iterations is None else max_iterations, C.byref(it), C.byref(res)))
        return it.value, res.value

    def solve_slae2(self, f2, solver_type=None, tolerance=None, max_iterations=None):
        """K [u, u2] = [f, f2] over one read of K per iteration (feahip_solve_slae2): (iters[2], resid[2]); the
        columns are read with solution() and solution2()."""
        f2 = np.ascontiguousarray(f2, dtype=np.float64)
        assert f2.shape == (self.ndof,)
        it, res = np.zeros(2, dtype=np.int32), np.zeros(2)
        d = self.deck
        self._chk(self._lib.feahip_solve_slae2(
            self._ctx, d.solver_type if solver_type is None else solver_type,
            d.solver_tolerance if tolerance is None else tolerance,
            d.solver_max_iter if max_iterations is None else max_iterations, _d(f2), _i(it), _d(res)))
        return it, res

    def get_solution2(self):
        u = np.zeros(self.ndof)
        self._chk(self._lib.feahip_get_solution2(self._ctx, _d(u)))
        return u

    solution2 = get_solution2

    def energy(self):
        t = C.c_double(0)
        self._chk(self._lib.feahip_energy(self._ctx, C.byref(t)))
        return t.value

    def update_nodes_with_solution(self, u=None):
        if u is None:
            self._chk(self._lib.feahip_update_nodes_with_solution(self._ctx, None))
        else:
            u = np.ascontiguousarray(u, dtype=np.float64)
            self._chk(self._lib.feahip_update_nodes_with_solution(self._ctx, _d(u)))

    def solve(self, load_increments=None, max_newton=None, modified_newton=None, desired_tolerance=None,
              solver_type=None, solver_tolerance=None, solver_max_iter=None, line_search=None):
        d = self.deck
        if line_search is not None:
            self.set_line_search(line_search)
        li = d.load_increments_count if load_increments is None else load_increments
        mn = d.max_newton_count if max_newton is None else max_newton
        cap = li * mn
        tol_log = np.zeros(cap)
        its = np.zeros(li, dtype=np.int32)
        done = C.c_int(0)
        self._chk(self._lib.feahip_solve(
            self._ctx, li, mn, int(d.modified_newton if modified_newton is None else modified_newton),
            d.desired_tolerance if desired_tolerance is None else desired_tolerance,
            d.solver_type if solver_type is None else solver_type,
            d.solver_tolerance if solver_tolerance is None else solver_tolerance,
            d.solver_max_iter if solver_max_iter is None else solver_max_iter,
            _d(tol_log), cap, _i(its), C.byref(done)))
        n = int(its[:max(done.value, 0) + (1 if done.value < li else 0)].sum())
        return done.value, its, tol_log[:n]

    def solve_arclength(self, lambda_max=None, max_steps=None, max_newton=None, desired_tolerance=None,
                        solver_type=None, solver_tolerance=None, solver_max_iter=None, check=True):
        """Arc-length continuation on the surface loads (feahip_solve_arclength).  Returns (steps done, lambda_log,
        its_log, tol_log, rc); with check=False a FEAHIP_ENOTCONVERGED comes back as rc instead of raising."""
        d = self.deck
        lmax = float(d.load_increments_count if lambda_max is None else lambda_max)
        ms = int(getattr(d, "arclength_max", 0) if max_steps is None else max_steps)
        mn = d.max_newton_count if max_newton is None else max_newton
        cap = ms * mn * 9
        lam, its, tol = np.zeros(max(ms, 1)), np.zeros(max(ms, 1), dtype=np.int32), np.zeros(max(cap, 1))
        done = C.c_int(0)
        rc = self._lib.feahip_solve_arclength(
            self._ctx, lmax, ms, mn, d.desired_tolerance if desired_tolerance is None else desired_tolerance,
            d.solver_type if solver_type is None else solver_type,
            d.solver_tolerance if solver_tolerance is None else solver_tolerance,
            d.solver_max_iter if solver_max_iter is None else solver_max_iter,
            _d(lam), _d(tol), cap, _i(its), C.byref(done))
        if check or rc != ENOTCONVERGED:
            self._chk(rc)
        n = max(done.value, 0)
        return n, lam[:n], its[:n], tol, rc

    # ---- consistent mass, body force, Newmark steps ------------------------
    def set_mass(self, rho):
        """feahip_set_mass with the mass rule of the element type (MASS_POINTS).  rho: one density, or one per material
        of the table in force; None (or an empty list) clears the mass, the body force, velocities and accelerations."""
        rho = np.zeros(0) if rho is None else np.ascontiguousarray(np.atleast_1d(rho), dtype=np.float64).ravel()
        if len(rho) == 0:
            self._chk(self._lib.feahip_set_mass(self._ctx, 0, None, 0, None, None, None))
            return
        gm = MASS_POINTS[self.deck.ele_type]
        w, forms, dforms = element_tables(self.deck.ele_type, gm)
        self._chk(self._lib.feahip_set_mass(self._ctx, len(rho), _d(rho), gm, _d(w), _d(forms), _d(dforms)))

    def mass_spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        assert len(x) == self.ndof
        y = np.zeros(self.ndof)
        self._chk(self._lib.feahip_mass_spmv(self._ctx, _d(x), _d(y)))
        return y

    def set_damping(self, alpha, beta=0.0):
        """feahip_set_damping: C = alpha M + beta K_d, K_d the plain tangent at the nodes in force (a snapshot, kept in a
        store as large as K when beta > 0).  (0, 0) clears it."""
        self._chk(self._lib.feahip_set_damping(self._ctx, float(alpha), float(beta)))

    def damping(self):
        a, b = C.c_double(0), C.c_double(0)
        self._chk(self._lib.feahip_get_damping(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def damping_spmv(self, v):
        """y = C v on the owned rows (zero on the others), as mass_spmv."""
        v = np.ascontiguousarray(v, dtype=np.float64).ravel()
        assert len(v) == self.ndof
        y = np.zeros(self.ndof)
        self._chk(self._lib.feahip_damping_spmv(self._ctx, _d(v), _d(y)))
        return y

    def set_body_force(self, b):
        b = None if b is None else np.ascontiguousarray(b, dtype=np.float64).reshape(3)
        self._chk(self._lib.feahip_set_body_force(self._ctx, None if b is None else _d(b)))

    def _node_get(self, fn):
        v = np.zeros((self.N, 3))
        self._chk(fn(self._ctx, _d(v)))
        return v

    def _node_set(self, fn, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        assert v.shape == (self.N, 3)
        self._chk(fn(self._ctx, _d(v)))

    def velocities(self):
        return self._node_get(self._lib.feahip_get_velocities)

    def set_velocities(self, v):
        self._node_set(self._lib.feahip_set_velocities, v)

    def accelerations(self):
        return self._node_get(self._lib.feahip_get_accelerations)

    def set_accelerations(self, a):
        self._node_set(self._lib.feahip_set_accelerations, a)

    def time(self):
        t = C.c_double(0)
        self._chk(self._lib.feahip_get_time(self._ctx, C.byref(t)))
        return t.value

    def set_time(self, t):
        self._chk(self._lib.feahip_set_time(self._ctx, float(t)))

    def consistent_acceleration(self, solver_type=None, tolerance=None, max_iterations=None):
        """Solves M a = lambda F_ext(x) - T(x) into the accelerations (collective on a group: one call drives it)."""
        d = self.deck
        self._chk(self._lib.feahip_consistent_acceleration(
            self._ctx, d.solver_type if solver_type is None else solver_type,
            d.solver_tolerance if tolerance is None else tolerance,
            d.solver_max_iter if max_iterations is None else max_iterations))

    def solve_dynamic(self, n_steps=None, dt=None, beta=None, gamma=None, dlambda=None, max_newton=None,
                      desired_tolerance=None, solver_type=None, solver_tolerance=None, solver_max_iter=None):
        """feahip_solve_dynamic; arguments left out come from the deck (its `dynamics`).  Returns (steps done, its_log,
        tol_log)."""
        d = self.deck
        dyn = getattr(d, "dynamics", None) or {}
        ns = int(dyn.get("steps", 0) if n_steps is None else n_steps)
        mn = d.max_newton_count if max_newton is None else max_newton
        cap = max(ns * mn, 1)
        tol_log, its, done = np.zeros(cap), np.zeros(max(ns, 1), dtype=np.int32), C.c_int(0)
        self._chk(self._lib.feahip_solve_dynamic(
            self._ctx, ns, float(dyn.get("dt", 0.0) if dt is None else dt), float(dyn.get("beta", 0.25) if beta is None else beta),
            float(dyn.get("gamma", 0.5) if gamma is None else gamma), float(dyn.get("dlambda", 0.0) if dlambda is None else dlambda),
            mn, d.desired_tolerance if desired_tolerance is None else desired_tolerance,
            d.solver_type if solver_type is None else solver_type,
            d.solver_tolerance if solver_tolerance is None else solver_tolerance,
            d.solver_max_iter if solver_max_iter is None else solver_max_iter, _d(tol_log), cap, _i(its), C.byref(done)))
        n = int(its[:min(done.value + 1, ns)].sum())
        return done.value, its[:ns], tol_log[:n]

    # ---- explicit steps on the lumped mass ---------------------------------
    def lumped_mass(self):
        """feahip_get_lumped_mass: ml[N], authoritative on the owned rows, zero elsewhere."""
        ml = np.zeros(self.N)
        self._chk(self._lib.feahip_get_lumped_mass(self._ctx, _d(ml)))
        return ml

    def stable_step(self):
        """feahip_stable_step: 2 / sqrt(Gershgorin bound) at the current nodes (collective on a group)."""
        dt = C.c_double(0)
        self._chk(self._lib.feahip_stable_step(self._ctx, C.byref(dt)))
        return dt.value

    def kinetic_energy(self):
        e = C.c_double(0)
        self._chk(self._lib.feahip_kinetic_energy(self._ctx, C.byref(e)))
        return e.value

    # ---- results ------------------------------------------------------------
    def nodal_stresses(self, material=-1):
        """feahip_get_nodal_stresses: (sig6[N][6] as xx yy zz xy yz xz, von_mises[N], weight[N]), the volume-weighted
        average over all elements (material = -1) or over those of one material; owned rows, zero elsewhere."""
        sig6, vm, wt = np.zeros((self.N, 6)), np.zeros(self.N), np.zeros(self.N)
        self._chk(self._lib.feahip_get_nodal_stresses(self._ctx, int(material), _d(sig6), _d(vm), _d(wt)))
        return sig6, vm, wt

    def strain_energy(self):
        """feahip_strain_energy (collective on a group)."""
        w = C.c_double(0)
        self._chk(self._lib.feahip_strain_energy(self._ctx, C.byref(w)))
        return w.value

    def nodal_energy(self):
        """feahip_get_nodal_energy: w_node[N], the shares W_e / npe of the owned rows."""
        wn = np.zeros(self.N)
        self._chk(self._lib.feahip_get_nodal_energy(self._ctx, _d(wn)))
        return wn

    def reactions(self):
        """feahip_get_reactions: r[3N], minus the unmasked residual on the prescribed dofs, zero elsewhere."""
        r = np.zeros(self.ndof)
        self._chk(self._lib.feahip_get_reactions(self._ctx, _d(r)))
        return r

    def solve_explicit(self, n_steps=None, dt=None, safety=None, restep=None, dlambda=None, check=True):
        """feahip_solve_explicit; arguments left out come from the deck (its `dynamics`).  Returns (steps done, dt_log
        of the steps taken) and, with check=False, the return code as a third item instead of raising on an inversion."""
        dyn = getattr(self.deck, "dynamics", None) or {}
        ns = int(dyn.get("steps", 0) if n_steps is None else n_steps)
        log, done = np.zeros(max(ns, 1)), C.c_int(0)
        rc = self._lib.feahip_solve_explicit(
            self._ctx, ns, float(dyn.get("dt", 0.0) if dt is None else dt),
            float(dyn.get("safety", 0.9) if safety is None else safety), int(dyn.get("restep", 0) if restep is None else restep),
            float(dyn.get("dlambda", 0.0) if dlambda is None else dlambda), _d(log), len(log), C.byref(done))
        if check or rc != ENOTCONVERGED:
            self._chk(rc)
        taken = log[:ns][log[:ns] > 0]
        return (done.value, taken) if check else (done.value, taken, rc)

    # ---- modal analysis ---------------------------------------------------
    def solve_modes(self, n_modes, tolerance=1e-8, max_iterations=1000, warm=False, check=True):
        """feahip_solve_modes: the n_modes lowest eigenpairs of K(x) phi = lambda M phi on the free dofs.  Returns
        (lam[n_modes] ascending = omega^2, resid[n_modes], Rayleigh-Ritz steps) and, with check=False, the return code
        as a fourth item instead of raising when the steps run out."""
        lam, res, it = np.zeros(max(int(n_modes), 1)), np.zeros(max(int(n_modes), 1)), C.c_int(0)
        rc = self._lib.feahip_solve_modes(self._ctx, int(n_modes), float(tolerance), int(max_iterations), int(bool(warm)),
                                          _d(lam), _d(res), C.byref(it))
        if check or rc != ENOTCONVERGED:
            self._chk(rc)
        return (lam, res, it.value) if check else (lam, res, it.value, rc)

    def solve_modes_sharded(self, n_modes, tolerance=1e-8, max_iterations=1000, warm=False, check=True):
        """feahip_solve_modes_sharded: solve_modes over the ranks of a sharded run.  Collective: every rank of an RCCL
        run (comm_init) makes the call; a member of an in-process group drives the whole group (FeaGroup.solve_modes).
        Returns what solve_modes returns, the same on every rank; modes() then gives this rank's rows, zero elsewhere."""
        lam, res, it = np.zeros(max(int(n_modes), 1)), np.zeros(max(int(n_modes), 1)), C.c_int(0)
        rc = self._lib.feahip_solve_modes_sharded(self._ctx, int(n_modes), float(tolerance), int(max_iterations),
                                                  int(bool(warm)), _d(lam), _d(res), C.byref(it))
        if check or rc != ENOTCONVERGED:
            self._chk(rc)
        return (lam, res, it.value) if check else (lam, res, it.value, rc)

    def modes(self, first=0, count=None):
        """feahip_get_modes: phi[count][3N] of the last solve_modes, M-orthonormal, zero on the prescribed dofs; all
        eight columns of the block are held (count=None: from `first` to the last).  After solve_modes_sharded: the
        rows this rank owns, zero on all others."""
        count = MODAL_COLS - first if count is None else count
        phi = np.zeros((max(int(count), 0), self.ndof))
        self._chk(self._lib.feahip_get_modes(self._ctx, int(first), int(count), _d(phi)))
        return phi

    def solve_modes_locked(self, n_modes, shift=0.0, tolerance=1e-8, max_iterations=4000, check=True):
        """feahip_solve_modes_locked: the n_modes <= 64 lowest eigenpairs of K(x) phi = lambda M phi by sweeps of the
        eight-column block with hard locking, on the pencil (K + shift M, M); lam is unshifted.  Returns (lam[n_modes]
        ascending, resid[n_modes], Rayleigh-Ritz steps over all sweeps, sweeps) and, with check=False, the return code as
        a fifth item instead of raising when the steps run out (lam and resid are NaN past the pairs locked by then:
        locked_count)."""
        lam, res = np.zeros(max(int(n_modes), 1)), np.zeros(max(int(n_modes), 1))
        it, sw = C.c_int(0), C.c_int(0)
        rc = self._lib.feahip_solve_modes_locked(self._ctx, int(n_modes), float(shift), float(tolerance), int(max_iterations),
                                                 _d(lam), _d(res), C.byref(it), C.byref(sw))
        if check or rc != ENOTCONVERGED:
            self._chk(rc)
        return (lam, res, it.value, sw.value) if check else (lam, res, it.value, sw.value, rc)

    def locked_count(self):
        """The modes in the locked store of the last solve_modes_locked (fewer than asked when its steps ran out)."""
        n = C.c_int(0)
        self._chk(self._lib.feahip_get_locked_count(self._ctx, C.byref(n)))
        return n.value

    def locked_lambda(self):
        """feahip_get_locked_lambda: the eigenvalues of the modes held, ascending and unshifted."""
        lam = np.zeros(self.locked_count())
        self._chk(self._lib.feahip_get_locked_lambda(self._ctx, 0, len(lam), _d(lam)))
        return lam

    def locked_modes(self, first=0, count=None):
        """feahip_get_locked_modes: phi[count][3N] of the last solve_modes_locked, M-orthonormal, zero on the prescribed
        dofs (count=None: from `first` to the last one locked)."""
        count = self.locked_count() - first if count is None else count
        phi = np.zeros((max(int(count), 0), self.ndof))
        self._chk(self._lib.feahip_get_locked_modes(self._ctx, int(first), int(count), _d(phi)))
        return phi

    def modal_deflate(self, q, x8):
        """x8 - Q (MQ' x8) by the two deflation kernels, MQ = mask(M Q) by the block product: q[n_locked][3N], x8[8][3N]."""
        q, x8 = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(x8, dtype=np.float64)
        assert q.ndim == 2 and q.shape[1] == self.ndof and x8.shape == (MODAL_COLS, self.ndof)
        out = np.zeros_like(x8)
        self._chk(self._lib.feahip_modal_deflate(self._ctx, len(q), _d(q), _d(x8), _d(out)))
        return out

    # ---- frequency response by mode superposition on the locked modes -----------
    def response_set_basis(self, lam, phi):
        """feahip_response_set_basis: installs the caller's M-orthonormal pairs lam[n], phi[n][3N] (n <= 64) into the locked
        store, as the modes of a solve with shift 0 (locked_modes returns them ascending in lam)."""
        lam, phi = np.ascontiguousarray(lam, dtype=np.float64), np.ascontiguousarray(phi, dtype=np.float64)
        assert lam.ndim == 1 and phi.shape == (len(lam), self.ndof)
        self._chk(self._lib.feahip_response_set_basis(self._ctx, len(lam), _d(lam), _d(phi)))

    def response_load(self, F, static_correction=True, solver_type=None, tolerance=None, max_iterations=None):
        """feahip_response_load: the participations q_k = phi_k' F of the real load F[3N] on the modes held and, with
        static_correction, K u_s = F by the context's PCG (the deck's solver settings where not given).  Returns
        (q[n_locked] ascending in lam, PCG iterations, PCG residual).  K, f and u hold other values afterwards."""
        d = self.deck
        F = np.ascontiguousarray(F, dtype=np.float64).reshape(self.ndof)
        q, it, res = np.zeros(MODAL_MAX_LOCKED), C.c_int(0), C.c_double(0)
        self._chk(self._lib.feahip_response_load(
            self._ctx, _d(F), int(bool(static_correction)), d.solver_type if solver_type is None else solver_type,
            d.solver_tolerance if tolerance is None else tolerance,
            d.solver_max_iter if max_iterations is None else max_iterations, _d(q), C.byref(it), C.byref(res)))
        return q[:self.locked_count()].copy(), it.value, res.value

    def response_static(self):
        """feahip_get_response_static: u_s[3N] of the load held (zero without the correction)."""
        u = np.zeros(self.ndof)
        self._chk(self._lib.feahip_get_response_static(self._ctx, _d(u)))
        return u

    def _zeta(self, zeta):
        if zeta is None:
            return None, None
        z = np.ascontiguousarray(np.broadcast_to(np.asarray(zeta, dtype=np.float64), (self.locked_count(),)))
        return z, _d(z)

    def response_sweep(self, omega, alpha=0.0, beta=0.0, zeta=None, probes=()):
        """feahip_response_sweep over the circular frequencies omega: (peak[3N] = max_j |u_i(w_j)|, peak_at[3N] = the
        lowest j that attains it, the complex curves [n_probe][n_freq] of the probe dofs 3 node + axis).  zeta: one
        ratio for all modes, one per mode, or None."""
        omega = np.ascontiguousarray(np.atleast_1d(omega), dtype=np.float64)
        pr = np.ascontiguousarray(probes, dtype=np.int32).reshape(-1)
        peak, at = np.zeros(self.ndof), np.zeros(self.ndof, dtype=np.int32)
        re, im = np.zeros((len(pr), len(omega))), np.zeros((len(pr), len(omega)))
        z, zp = self._zeta(zeta)
        self._chk(self._lib.feahip_response_sweep(self._ctx, len(omega), _d(omega), float(alpha), float(beta), zp, _d(peak),
                                                  _i(at), len(pr), _i(pr), _d(re), _d(im)))
        return peak, at, re + 1j * im

    def response_field(self, omega, alpha=0.0, beta=0.0, zeta=None):
        """feahip_response_field: the complex amplitude u[3N] at one circular frequency."""
        re, im = np.zeros(self.ndof), np.zeros(self.ndof)
        z, zp = self._zeta(zeta)
        self._chk(self._lib.feahip_response_field(self._ctx, float(omega), float(alpha), float(beta), zp, _d(re), _d(im)))
        return re + 1j * im

    # ---- transient response by mode superposition, base excitation -------------
    def response_base_load(self, direction, static_correction=True, solver_type=None, tolerance=None, max_iterations=None):
        """feahip_response_base_load: the load F = -M r of a rigid base acceleration along `direction` (r the translation on
        all dofs), held like the load of response_load.  Returns (q[n_locked], the participation factors gamma = -q, the
        effective masses gamma^2, the total mass r' M r, PCG iterations, PCG residual)."""
        d = self.deck
        r = np.ascontiguousarray(direction, dtype=np.float64).reshape(3)
        q, gamma, eff = np.zeros(MODAL_MAX_LOCKED), np.zeros(MODAL_MAX_LOCKED), np.zeros(MODAL_MAX_LOCKED)
        total, it, res = C.c_double(0), C.c_int(0), C.c_double(0)
        self._chk(self._lib.feahip_response_base_load(
            self._ctx, _d(r), int(bool(static_correction)), d.solver_type if solver_type is None else solver_type,
            d.solver_tolerance if tolerance is None else tolerance,
            d.solver_max_iter if max_iterations is None else max_iterations, _d(q), _d(gamma), _d(eff), C.byref(total),
            C.byref(it), C.byref(res)))
        n = self.locked_count()
        return q[:n].copy(), gamma[:n].copy(), eff[:n].copy(), total.value, it.value, res.value

    def response_transient(self, g, dt, alpha=0.0, beta=0.0, zeta=None, quantity=0, probes=(), snapshots=()):
        """feahip_response_transient under the load held times g(t), g[n_steps + 1] at t_n = n dt: (peak[3N] = max_n
        |u_i(t_n)|, peak_at[3N] = the lowest step that attains it, the histories [n_probe][n_steps + 1] of the probe dofs
        3 node + axis, the fields [n_snap][3N] at the snapshot steps).  quantity 0 displacement, 1 velocity, 2 acceleration
        relative to the base."""
        g = np.ascontiguousarray(np.atleast_1d(g), dtype=np.float64)
        pr = np.ascontiguousarray(probes, dtype=np.int32).reshape(-1)
        sn = np.ascontiguousarray(snapshots, dtype=np.int32).reshape(-1)
        peak, at = np.zeros(self.ndof), np.zeros(self.ndof, dtype=np.int32)
        hist, snap = np.zeros((len(pr), len(g))), np.zeros((len(sn), self.ndof))
        z, zp = self._zeta(zeta)
        self._chk(self._lib.feahip_response_transient(self._ctx, len(g) - 1, float(dt), _d(g), float(alpha), float(beta), zp,
                                                      int(quantity), _d(peak), _i(at), len(pr), _i(pr), _d(hist), len(sn),
                                                      _i(sn), _d(snap)))
        return peak, at, hist, snap

    # ---- response spectrum and random vibration: one quadratic form per dof ------
    def _held(self):
        """The modes held, or None where there are none (the entry called then says why)."""
        n = C.c_int(0)
        return n.value if self._lib.feahip_get_locked_count(self._ctx, C.byref(n)) == 0 else None

    def response_combine(self, C_, b=None, s=0.0, absolute=False):
        """feahip_response_combine: out[3N] = sqrt(max(0, x' C x + 2 u_s (b' x) + s u_s^2)) on every dof, x its values of the
        modes held (|x| with absolute), u_s the static correction of the load held.  C[n_locked][n_locked] symmetric to the
        bit and b[n_locked] by ascending mode."""
        n = self._held()
        Cm = np.ascontiguousarray(C_, dtype=np.float64)
        bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        assert n is None or (Cm.shape == (n, n) and (bb is None or bb.shape == (n,)))
        out = np.zeros(self.ndof)
        self._chk(self._lib.feahip_response_combine(self._ctx, _d(Cm), None if bb is None else _d(bb), float(s),
                                                    int(bool(absolute)), _d(out)))
        return out

    def response_random(self, omega, S, alpha=0.0, beta=0.0, zeta=None, quantity=0):
        """feahip_response_random: (rms[3N], the modal covariance C[n_locked][n_locked]) of the quantity (0 displacement, 1
        velocity, 2 acceleration) under the load held times a load factor of one-sided PSD S(omega) per rad/s, omega
        strictly ascending (host_random_grid makes a grid that resolves the peaks)."""
        omega, S = np.ascontiguousarray(omega, dtype=np.float64), np.ascontiguousarray(S, dtype=np.float64)
        assert omega.ndim == 1 and omega.shape == S.shape
        n = self._held()
        rms, cov = np.zeros(self.ndof), np.zeros((n or MODAL_MAX_LOCKED,) * 2)
        z, zp = (None, None) if n is None else self._zeta(zeta)
        self._chk(self._lib.feahip_response_random(self._ctx, len(omega), _d(omega), _d(S), float(alpha), float(beta), zp,
                                                   int(quantity), _d(rms), _d(cov)))
        return rms, cov

    def response_spectrum(self, w, sa, rule=SRSS, alpha=0.0, beta=0.0, zeta=None, zpa=0.0, quantity=0, loglog=False):
        """feahip_response_spectrum: (peak[3N], the peak modal values a[n_locked]) under the response spectrum sa(w), w in
        rad/s, with the load held (a base load: q_k = -gamma_k), combined by rule SRSS, CQC or ABS; zpa > 0 adds the
        missing mass of a load held with the static correction."""
        w, sa = np.ascontiguousarray(w, dtype=np.float64), np.ascontiguousarray(sa, dtype=np.float64)
        assert w.ndim == 1 and w.shape == sa.shape
        n = self._held()
        peak, a = np.zeros(self.ndof), np.zeros(MODAL_MAX_LOCKED)
        z, zp = (None, None) if n is None else self._zeta(zeta)
        self._chk(self._lib.feahip_response_spectrum(self._ctx, len(w), _d(w), _d(sa), int(bool(loglog)), int(rule),
                                                     float(alpha), float(beta), zp, float(zpa), int(quantity), _d(peak), _d(a)))
        return peak, a[:n or 0].copy()

    # ---- stress from mode superposition: modal stresses, RMS and peak von Mises -----
    def stress_increment(self, du, material=-1):
        """feahip_stress_increment: sig6[N][6] (xx yy zz xy yz xz), the nodal stress the displacement increment du[3N]
        causes at the current nodes with the weights of nodal_stresses held fixed; material = -1 takes all elements."""
        du = np.ascontiguousarray(du, dtype=np.float64).reshape(-1)
        assert du.shape == (self.ndof,)
        sig6 = np.zeros((self.ndof // 3, 6))
        self._chk(self._lib.feahip_stress_increment(self._ctx, _d(du), int(material), _d(sig6)))
        return sig6

    def response_stress_basis(self, material=-1):
        """feahip_response_stress_basis: builds the stress store of the modes held at the current nodes, and T_s of the
        load held with the static correction."""
        self._chk(self._lib.feahip_response_stress_basis(self._ctx, int(material)))

    def modal_stresses(self, first=0, count=None):
        """feahip_get_modal_stresses: sig6[count][N][6] of the modes held, by ascending lam."""
        n = self._held()
        count = (n or 0) - first if count is None else count
        out = np.zeros((max(count, 0), self.ndof // 3, 6))
        self._chk(self._lib.feahip_get_modal_stresses(self._ctx, int(first), int(count), _d(out)))
        return out

    def response_static_stress(self):
        """feahip_get_response_static_stress: T_s[N][6], the stress of u_s (zero without the correction)."""
        out = np.zeros((self.ndof // 3, 6))
        self._chk(self._lib.feahip_get_response_static_stress(self._ctx, _d(out)))
        return out

    def response_stress_field(self, coef, cs=0.0):
        """feahip_response_stress_field: (sig6[N][6] = cs T_s + sum_k coef_k T_k, its von Mises stress [N]), coef by
        ascending mode: the stress of one row of host_response_coefficients or host_transient_coefficients."""
        n = self._held()
        co = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
        assert n is None or len(co) >= n
        sig6, vm = np.zeros((self.ndof // 3, 6)), np.zeros(self.ndof // 3)
        self._chk(self._lib.feahip_response_stress_field(self._ctx, _d(co), float(cs), _d(sig6), _d(vm)))
        return sig6, vm

    def response_stress_combine(self, C_, b=None, s=0.0):
        """feahip_response_stress_combine: (out6[N][6], vm[N]) of the form (C, b, s) on the modal stresses: the root of the
        form on each component, and the von Mises root of its own nine forms."""
        n = self._held()
        Cm = np.ascontiguousarray(C_, dtype=np.float64)
        bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        assert n is None or (Cm.shape == (n, n) and (bb is None or bb.shape == (n,)))
        out6, vm = np.zeros((self.ndof // 3, 6)), np.zeros(self.ndof // 3)
        self._chk(self._lib.feahip_response_stress_combine(self._ctx, _d(Cm), None if bb is None else _d(bb), float(s),
                                                           _d(out6), _d(vm)))
        return out6, vm

    def response_stress_random(self, omega, S, alpha=0.0, beta=0.0, zeta=None):
        """feahip_response_stress_random: (rms6[N][6], the RMS von Mises stress [N], the modal covariance) under the load
        held times a load factor of one-sided PSD S(omega)."""
        omega, S = np.ascontiguousarray(omega, dtype=np.float64), np.ascontiguousarray(S, dtype=np.float64)
        assert omega.ndim == 1 and omega.shape == S.shape
        n = self._held()
        rms6, vm, cov = np.zeros((self.ndof // 3, 6)), np.zeros(self.ndof // 3), np.zeros((n or MODAL_MAX_LOCKED,) * 2)
        z, zp = (None, None) if n is None else self._zeta(zeta)
        self._chk(self._lib.feahip_response_stress_random(self._ctx, len(omega), _d(omega), _d(S), float(alpha), float(beta),
                                                          zp, _d(rms6), _d(vm), _d(cov)))
        return rms6, vm, cov

    def response_stress_moments(self, C4, b4=None, s4=None):
        """feahip_response_stress_moments: moments[N][7][4], four forms (C4[k], b4[k], s4[k]) on the six stress components and
        on the von Mises combination of the nine forms of every node, in one launch: max(0, form), no root.  b4 and s4, or
        single entries of them, may be None: zero."""
        n = self._held()
        Cm = np.ascontiguousarray(C4, dtype=np.float64)
        assert Cm.ndim == 3 and Cm.shape[0] == 4 and (n is None or Cm.shape[1:] == (n, n))
        m = Cm.shape[1]
        bb = None if b4 is None else np.ascontiguousarray([np.zeros(m) if b is None else np.asarray(b, dtype=np.float64) for b in b4])
        ss = None if s4 is None else np.ascontiguousarray([0.0 if v is None else float(v) for v in s4], dtype=np.float64)
        assert (bb is None or bb.shape == (4, m)) and (ss is None or ss.shape == (4,))
        mom = np.zeros((self.ndof // 3, 7, 4))
        self._chk(self._lib.feahip_response_stress_moments(self._ctx, _d(Cm), None if bb is None else _d(bb),
                                                           None if ss is None else _d(ss), _d(mom)))
        return mom

    def response_stress_fatigue(self, omega, S, alpha=0.0, beta=0.0, zeta=None, sn_exponent=3.0, sn_coefficient=1.0):
        """feahip_response_stress_fatigue: (moments[N][7][4], rates[N][7][2], damage[N][7][3], status[N][7]) under the load
        held times a load factor of one-sided PSD S(omega): the spectral moments m0, m1, m2, m4 of the six stress components
        and of the equivalent von Mises process, nu0 and nup in cycles per unit time, the damage per unit time on the
        S-N curve N s^b = A (s the stress amplitude) by FATIGUE_DAMAGE, and the status bits FATIGUE_*."""
        omega, S = np.ascontiguousarray(omega, dtype=np.float64), np.ascontiguousarray(S, dtype=np.float64)
        assert omega.ndim == 1 and omega.shape == S.shape
        n = self._held()
        N = self.ndof // 3
        mom, rates, damage, status = np.zeros((N, 7, 4)), np.zeros((N, 7, 2)), np.zeros((N, 7, 3)), np.zeros((N, 7), dtype=np.int32)
        z, zp = (None, None) if n is None else self._zeta(zeta)
        self._chk(self._lib.feahip_response_stress_fatigue(self._ctx, len(omega), _d(omega), _d(S), float(alpha), float(beta), zp,
                                                           float(sn_exponent), float(sn_coefficient), _d(mom), _d(rates),
                                                           _d(damage), _i(status)))
        return mom, rates, damage, status

    def response_stress_spectrum(self, w, sa, rule=SRSS, alpha=0.0, beta=0.0, zeta=None, zpa=0.0, loglog=False, von_mises=None):
        """feahip_response_stress_spectrum: (peak6[N][6], the peak von Mises stress [N] or None, the peak modal values)
        under the response spectrum sa(w).  Under ABS the components take |T| and there is no von Mises peak (von_mises
        defaults to rule != ABS; asking for it under ABS is refused)."""
        w, sa = np.ascontiguousarray(w, dtype=np.float64), np.ascontiguousarray(sa, dtype=np.float64)
        assert w.ndim == 1 and w.shape == sa.shape
        n = self._held()
        want_vm = (rule != ABS) if von_mises is None else bool(von_mises)
        peak6, a = np.zeros((self.ndof // 3, 6)), np.zeros(MODAL_MAX_LOCKED)
        vm = np.zeros(self.ndof // 3) if want_vm else None
        z, zp = (None, None) if n is None else self._zeta(zeta)
        self._chk(self._lib.feahip_response_stress_spectrum(self._ctx, len(w), _d(w), _d(sa), int(bool(loglog)), int(rule),
                                                            float(alpha), float(beta), zp, float(zpa), _d(peak6),
                                                            None if vm is None else _d(vm), _d(a)))
        return peak6, vm, a[:n or 0].copy()

    # ---- stress peaks over a sweep or a transient, one launch each ----------------
    def response_stress_sweep(self, omega, alpha=0.0, beta=0.0, zeta=None, probes=()):
        """feahip_response_stress_sweep over the circular frequencies omega: (peak6[N][6] = max_j |s_c(w_j)|, peak6_at[N][6],
        vm[N] = the largest von Mises stress over the cycle and the frequencies, vm_at[N], the complex curves
        [n_probe][n_freq][6] of the probe nodes); every _at the lowest j that attains its peak."""
        omega = np.ascontiguousarray(np.atleast_1d(omega), dtype=np.float64)
        pr = np.ascontiguousarray(probes, dtype=np.int32).reshape(-1)
        N = self.ndof // 3
        peak6, at6 = np.zeros((N, 6)), np.zeros((N, 6), dtype=np.int32)
        vm, vat = np.zeros(N), np.zeros(N, dtype=np.int32)
        re, im = np.zeros((len(pr), len(omega), 6)), np.zeros((len(pr), len(omega), 6))
        z, zp = (None, None) if self._held() is None else self._zeta(zeta)
        self._chk(self._lib.feahip_response_stress_sweep(self._ctx, len(omega), _d(omega), float(alpha), float(beta), zp,
                                                         _d(peak6), _i(at6), _d(vm), _i(vat), len(pr), _i(pr), _d(re), _d(im)))
        return peak6, at6, vm, vat, re + 1j * im

    def response_stress_transient(self, g, dt, alpha=0.0, beta=0.0, zeta=None, probes=()):
        """feahip_response_stress_transient under the load held times g(t), g[n_steps + 1] at t_n = n dt: (peak6[N][6] =
        max_n |sigma_c(t_n)|, peak6_at[N][6], vm[N] = the largest von Mises stress, vm_at[N], the histories
        [n_probe][n_steps + 1][6] of the probe nodes); every _at the lowest step that attains its peak."""
        g = np.ascontiguousarray(np.atleast_1d(g), dtype=np.float64)
        pr = np.ascontiguousarray(probes, dtype=np.int32).reshape(-1)
        N = self.ndof // 3
        peak6, at6 = np.zeros((N, 6)), np.zeros((N, 6), dtype=np.int32)
        vm, vat = np.zeros(N), np.zeros(N, dtype=np.int32)
        hist = np.zeros((len(pr), len(g), 6))
        z, zp = (None, None) if self._held() is None else self._zeta(zeta)
        self._chk(self._lib.feahip_response_stress_transient(self._ctx, len(g) - 1, float(dt), _d(g), float(alpha), float(beta),
                                                             zp, _d(peak6), _i(at6), _d(vm), _i(vat), len(pr), _i(pr), _d(hist)))
        return peak6, at6, vm, vat, hist

    # ---- rainflow counting of a transient ----------------------------------------
    def response_stress_rainflow(self, g, dt, alpha=0.0, beta=0.0, zeta=None, sn_exponent=3.0, sn_coefficient=1.0, depth=32,
                                 projections=None, probes=()):
        """feahip_response_stress_rainflow under the load held times g(t), g[n_steps + 1] at t_n = n dt: the rainflow count
        of the six stress components of every node and of the linear projections given ([n_proj][6], plane_projections
        makes those of planes), as a dict of damage, cycles, max_range, status, depth_used, each [N][6 + n_proj], and
        probes, the histories [n_probe][n_steps + 1][6 + n_proj] of the probe nodes.  Damage is Miner's sum on the S-N curve
        N s^b = A (s the stress amplitude); status has the bits RAINFLOW_*."""
        g = np.ascontiguousarray(np.atleast_1d(g), dtype=np.float64)
        pr = np.ascontiguousarray(probes, dtype=np.int32).reshape(-1)
        pj = None if projections is None else np.ascontiguousarray(projections, dtype=np.float64)
        assert pj is None or (pj.ndim == 2 and pj.shape[1] == 6)
        n_proj = 0 if pj is None else pj.shape[0]
        N, W = self.ndof // 3, 6 + n_proj
        damage, cycles, max_range = np.zeros((N, W)), np.zeros((N, W)), np.zeros((N, W))
        status, used = np.zeros((N, W), dtype=np.int32), np.zeros((N, W), dtype=np.int32)
        hist = np.zeros((len(pr), len(g), W))
        z, zp = (None, None) if self._held() is None else self._zeta(zeta)
        self._chk(self._lib.feahip_response_stress_rainflow(self._ctx, len(g) - 1, float(dt), _d(g), float(alpha), float(beta), zp,
                                                            float(sn_exponent), float(sn_coefficient), int(depth), n_proj,
                                                            None if n_proj == 0 else _d(pj), _d(damage), _d(cycles),
                                                            _d(max_range), _i(status), _i(used), len(pr), _i(pr), _d(hist)))
        return dict(damage=damage, cycles=cycles, max_range=max_range, status=status, depth_used=used, probes=hist)

    # ---- linear buckling ---------------------------------------------------
    def solve_buckling(self, n_modes, tolerance=1e-8, max_iterations=2000, check=True):
        """feahip_solve_buckling: the n_modes lowest eigenpairs of K_sigma(x) phi = nu K(x) phi on the free dofs.  Returns
        (factor[n_modes] = 1 - 1/nu where nu < 0 and +infinity elsewhere, nu[n_modes] ascending, resid[n_modes],
        Rayleigh-Ritz steps) and, with check=False, the return code as a fifth item instead of raising when the steps
        run out or K is not positive definite."""
        n = max(int(n_modes), 1)
        fac, nu, res, it = np.zeros(n), np.zeros(n), np.zeros(n), C.c_int(0)
        rc = self._lib.feahip_solve_buckling(self._ctx, int(n_modes), float(tolerance), int(max_iterations), _d(fac), _d(nu),
                                             _d(res), C.byref(it))
        if check or rc != ENOTCONVERGED:
            self._chk(rc)
        return (fac, nu, res, it.value) if check else (fac, nu, res, it.value, rc)

    def buckling_modes(self, first=0, count=None):
        """feahip_get_buckling_modes: phi[count][3N] of the last solve_buckling, K-orthonormal, zero on the prescribed
        dofs; all eight columns of the block are held (count=None: from `first` to the last)."""
        count = MODAL_COLS - first if count is None else count
        phi = np.zeros((max(int(count), 0), self.ndof))
        self._chk(self._lib.feahip_get_buckling_modes(self._ctx, int(first), int(count), _d(phi)))
        return phi

    def geometric_spmv(self, x):
        """y = K_sigma(current nodes) x, unmasked (feahip_geometric_spmv; K_sigma is assembled on each call)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        assert x.size == self.ndof
        y = np.zeros(self.ndof)
        self._chk(self._lib.feahip_geometric_spmv(self._ctx, _d(x), _d(y)))
        return y

    def spmm_km(self, x8):
        """[K X, mask(M X)] of eight columns in one pass over K's pattern; x8 and both results are [8][3N]."""
        x8 = np.ascontiguousarray(x8, dtype=np.float64)
        assert x8.shape == (MODAL_COLS, self.ndof)
        y8, z8 = np.zeros_like(x8), np.zeros_like(x8)
        self._chk(self._lib.feahip_spmm_km(self._ctx, _d(x8), _d(y8), _d(z8)))
        return y8, z8

    # ---- surface loads ---------------------------------------------------
    def set_surface_loads(self, faces, kind, values):
        """Replaces the loaded faces (an empty list clears them): faces[F][nodes per face] in the caller's node ids,
        any order; kind[F] LOAD_PRESSURE / LOAD_TRACTION; values[F][3] (pressure in [0], or t0)."""
        kind = np.ascontiguousarray(kind, dtype=np.int32).reshape(-1)
        n = len(kind)
        faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(n, -1) if n else np.zeros((0, 1), dtype=np.int32)
        values = np.ascontiguousarray(values, dtype=np.float64).reshape(n, 3) if n else np.zeros((0, 3))
        self._chk(self._lib.feahip_set_surface_loads(self._ctx, n, faces.shape[1] if n else 0, _i(faces), _i(kind), _d(values)))

    def surface_forces(self):
        """load factor x F_ext at the current nodes, [3N] in the caller's dof order."""
        f = np.zeros(self.ndof)
        self._chk(self._lib.feahip_get_surface_forces(self._ctx, _d(f)))
        return f

    # ---- contact with rigid obstacles ---------------------------------------
    def set_contact(self, faces, obstacles, penalty, augment_max=0, gap_tolerance=0.0):
        """feahip_set_contact: faces[F][nodes per face] as set_surface_loads takes them; obstacles a list of dicts
        (kind, point | center, normal | axis | direction, radius, travel) or tuples (kind, point, direction, radius,
        travel).  No faces or no obstacles clears the contact."""
        faces = np.asarray(faces, dtype=np.int32)
        n = len(faces) if faces.size else 0
        faces = np.ascontiguousarray(faces.reshape(n, -1)) if n else np.zeros((0, 1), dtype=np.int32)
        kind, geom = obstacle_arrays(obstacles)
        self._chk(self._lib.feahip_set_contact(self._ctx, n, faces.shape[1] if n else 0, _i(faces), len(kind), _i(kind), _d(geom),
                                               float(penalty), int(augment_max), float(gap_tolerance)))

    def contact_nodes(self):
        """(nodes[n] ascending in this solver's node ids, weights[n]) of the contact nodes the context owns."""
        n = C.c_int(0)
        self._chk(self._lib.feahip_get_contact_nodes(self._ctx, C.byref(n), None, None))
        nodes, w = np.zeros(n.value, dtype=np.int32), np.zeros(n.value)
        if n.value:
            self._chk(self._lib.feahip_get_contact_nodes(self._ctx, C.byref(n), _i(nodes), _d(w)))
        return nodes, w

    def contact_obstacles(self):
        """feahip_get_contact_obstacles: the obstacles of the contact in force (0 without one)."""
        n = C.c_int(0)
        self._chk(self._lib.feahip_get_contact_obstacles(self._ctx, C.byref(n)))
        return n.value

    def contact_multipliers(self):
        """mu[n][obstacles] in the node order of contact_nodes()."""
        n = len(self.contact_nodes()[0])
        mu = np.zeros((n, self.contact_obstacles()))
        if mu.size:
            self._chk(self._lib.feahip_get_contact_multipliers(self._ctx, _d(mu)))
        return mu

    def set_contact_multipliers(self, mu):
        n = len(self.contact_nodes()[0])
        mu = np.ascontiguousarray(mu, dtype=np.float64).reshape(n, self.contact_obstacles())
        if mu.size:
            self._chk(self._lib.feahip_set_contact_multipliers(self._ctx, _d(mu)))

    def contact_forces(self):
        """F_c at the current nodes, [3N] in the caller's dof order."""
        f = np.zeros(self.ndof)
        self._chk(self._lib.feahip_get_contact_forces(self._ctx, _d(f)))
        return f

    def contact_status(self):
        """(gap[N]: the smallest over the obstacles, +inf away from the contact nodes; pressure[N]: the summed t)."""
        gap, t = np.zeros(self.N), np.zeros(self.N)
        self._chk(self._lib.feahip_get_contact_status(self._ctx, _d(gap), _d(t)))
        return gap, t

    def contact_info(self):
        """feahip_contact_info (collective on a group): dict(active, max_penetration, force, potential)."""
        o = np.zeros(4)
        self._chk(self._lib.feahip_contact_info(self._ctx, _d(o)))
        return {"active": int(o[0]), "max_penetration": o[1], "force": o[2], "potential": o[3]}

    def contact_augment(self):
        """feahip_contact_augment (collective on a group): the largest penetration before the multiplier update."""
        p = C.c_double(0)
        self._chk(self._lib.feahip_contact_augment(self._ctx, C.byref(p)))
        return p.value

    def load_factor(self):
        v = C.c_double(0)
        self._chk(self._lib.feahip_get_load_factor(self._ctx, C.byref(v)))
        return v.value

    def set_load_factor(self, lam):
        self._chk(self._lib.feahip_set_load_factor(self._ctx, lam))

    # ---- views -----------------------------------------------------------
    def set_nodes(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (self.N, 3)
        self._chk(self._lib.feahip_set_nodes(self._ctx, _d(x)))

    def nodes(self):
        x = np.zeros((self.N, 3))
        self._chk(self._lib.feahip_get_nodes(self._ctx, _d(x)))
        return x

    def shape_gradients(self):
        """(grads[E][G][3][npe], detJ[E][G]) of the current configuration."""
        g = np.zeros((self.E, self.G, 3, self.npe))
        d = np.zeros((self.E, self.G))
        self._chk(self._lib.feahip_get_shape_gradients(self._ctx, _d(g), _d(d)))
        return g, d

    def forces(self):
        f = np.zeros(self.ndof)
        self._chk(self._lib.feahip_get_forces(self._ctx, _d(f)))
        return f

    def set_forces(self, f):
        f = np.ascontiguousarray(f, dtype=np.float64)
        assert f.shape == (self.ndof,)
        self._chk(self._lib.feahip_set_forces(self._ctx, _d(f)))

    def solution(self):
        u = np.zeros(self.ndof)
        self._chk(self._lib.feahip_get_solution(self._ctx, _d(u)))
        return u

    def graddefs(self):
        F = np.zeros((self.E, self.G, 3, 3))
        self._chk(self._lib.feahip_get_graddefs(self._ctx, _d(F)))
        return F

    def stresses(self):
        S = np.zeros((self.E, self.G, 3, 3))
        self._chk(self._lib.feahip_get_stresses(self._ctx, _d(S)))
        return S

    def matrix_yale(self):
        nnz = C.c_longlong(0)
        self._chk(self._lib.feahip_matrix_nnz(self._ctx, C.byref(nnz)))
        off = np.zeros(self.ndof + 1, dtype=np.int32)
        idx = np.zeros(nnz.value, dtype=np.int32)
        val = np.zeros(nnz.value)
        self._chk(self._lib.feahip_get_matrix_yale(self._ctx, _i(off), _i(idx), _d(val)))
        return off, idx, val

    def matrix_yale64(self):
        """The same with 64-bit offsets (feahip_get_matrix_yale refuses 2^31 or more scalar non-zeros)."""
        nnz = C.c_longlong(0)
        self._chk(self._lib.feahip_matrix_nnz(self._ctx, C.byref(nnz)))
        off = np.zeros(self.ndof + 1, dtype=np.int64)
        idx = np.zeros(nnz.value, dtype=np.int32)
        val = np.zeros(nnz.value)
        self._chk(self._lib.feahip_get_matrix_yale64(self._ctx, off.ctypes.data_as(C.POINTER(C.c_longlong)), _i(idx), _d(val)))
        return off, idx, val

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros(self.ndof)
        self._chk(self._lib.feahip_spmv(self._ctx, _d(x), _d(y)))
        return y

    def spmv2(self, x2):
        """[y, y2] = K [x, x2] in one pass over K; x2 and the result are [2][3N]."""
        x2 = np.ascontiguousarray(x2, dtype=np.float64)
        assert x2.shape == (2, self.ndof)
        y2 = np.zeros((2, self.ndof))
        self._chk(self._lib.feahip_spmv2(self._ctx, _d(x2), _d(y2)))
        return y2

    # ---- tuning / measurement ------------------------------------------
    def set_preconditioner(self, kind):
        """0 block-Jacobi, 1 multigrid, 2 multigrid plus a coarse level across the ranks (feahip_set_preconditioner)."""
        self._chk(self._lib.feahip_set_preconditioner(self._ctx, kind))
        self.preconditioner = kind

    def coarse_info(self):
        """The coarse level of preconditioner 2 for the current K (feahip_coarse_info): dict of COARSE_INFO_KEYS plus
        agg [owned rows] (global aggregate of every owned row, in the context's row order) and centroids
        [aggregates][3] of all aggregates."""
        o = (C.c_longlong * 8)()
        self._chk(self._lib.feahip_coarse_info(self._ctx, o, None, None))
        d = dict(zip(COARSE_INFO_KEYS, [int(v) for v in o]))
        agg = np.zeros(max(d["owned_rows"], 1), dtype=np.int32)
        cent = np.zeros((max(d["aggregates"], 1), 3))
        self._chk(self._lib.feahip_coarse_info(self._ctx, o, _i(agg), _d(cent)))
        d.update(zip(COARSE_INFO_KEYS, [int(v) for v in o]))
        d["agg"], d["centroids"] = agg[:d["owned_rows"]], cent[:d["aggregates"]]
        return d

    def coarse_matrix(self):
        """The all-reduced Phi' K Phi of preconditioner 2 for the current K, [unknowns][unknowns]."""
        n = self.coarse_info()["unknowns"]
        A = np.zeros((n, n))
        self._chk(self._lib.feahip_coarse_matrix(self._ctx, _d(A)))
        return A

    def apply_preconditioner(self, r):
        """z = M^-1 r with the preconditioner the next PCG solve would use (set_preconditioner), for the current K."""
        r = np.ascontiguousarray(r, dtype=np.float64).ravel()
        z = np.zeros(self.ndof)
        self._chk(self._lib.feahip_apply_preconditioner(self._ctx, _d(r), _d(z)))
        return z

    def amg_info(self):
        """The multigrid hierarchy's parameters and which paths its one-workgroup tail takes (feahip_amg_info)."""
        o = (C.c_longlong * 16)()
        over = C.c_double(0)
        self._chk(self._lib.feahip_amg_info(self._ctx, o, C.byref(over)))
        d = dict(zip(AMG_INFO_KEYS, [int(v) for v in o]))
        d["tail_entry"] = TAIL_ENTRY[d["tail_entry"]]
        d["coarse_f32"], d["fused_post"], d["tail_cop"], d["tail_blob"] = (bool(d[k]) for k in ("coarse_f32", "fused_post", "tail_cop", "tail_blob"))
        d["tail_lds_levels"] = [l for l in range(d["levels"]) if d["tail_lds_levels"] >> l & 1]
        d["over"] = over.value
        return d

    def amg_level(self, level):
        """One level of the hierarchy as stored (feahip_amg_level): dict N, nnzb, Nc, bits, omega, rowptr, colidx,
        K [nnzb][3][3] widened to double, agg, doff [N][3], type.  Level 0 in the caller's node ids."""
        cnt = (C.c_longlong * 4)()
        om = C.c_double(0)
        self._chk(self._lib.feahip_amg_level(self._ctx, level, cnt, C.byref(om), None, None, None, None, None, None))
        N, nnzb, Nc, bits = (int(v) for v in cnt)
        rowptr, colidx = np.zeros(N + 1, dtype=np.int32), np.zeros(max(nnzb, 1), dtype=np.int32)
        K, agg = np.zeros((max(nnzb, 1), 3, 3)), np.zeros(max(N, 1), dtype=np.int32)
        doff, typ = np.zeros((max(N, 1), 3)), np.zeros(max(N, 1), dtype=np.int32)
        self._chk(self._lib.feahip_amg_level(self._ctx, level, cnt, C.byref(om), _i(rowptr), _i(colidx), _d(K), _i(agg),
                                             _d(doff), _i(typ)))
        return dict(N=N, nnzb=nnzb, Nc=Nc, bits=bits, omega=om.value, rowptr=rowptr, colidx=colidx[:nnzb], K=K[:nnzb],
                    agg=agg[:N], doff=doff[:N], type=typ[:N])

    def set_pcg_variant(self, variant):
        self._chk(self._lib.feahip_set_pcg_variant(self._ctx, variant))

    def set_line_search(self, max_iterations):
        self._chk(self._lib.feahip_set_line_search(self._ctx, max_iterations))

    def set_assembly(self, strategy):
        self._chk(self._lib.feahip_set_assembly(self._ctx, strategy))

    def set_row_shard(self, rank, nranks):
        self._chk(self._lib.feahip_set_row_shard(self._ctx, rank, nranks))

    def owned_rows(self):
        """[row0, row1) in LIBRARY node ids (see node_numbering / owned_nodes)."""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self._lib.feahip_owned_rows(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def node_numbering(self):
        """library id of every caller's node (the identity when the library kept the caller's numbering)."""
        out = np.empty(self.N, dtype=np.int32)
        self._chk(self._lib.feahip_node_numbering(self._ctx, _i(out)))
        return out

    def owned_nodes(self):
        """the caller's ids of the nodes this rank owns, ascending."""
        r0, r1 = self.owned_rows()
        lib = self.node_numbering()
        return np.nonzero((lib >= r0) & (lib < r1))[0]

    def owned_dofs(self):
        """the caller's dof indices (node * 3 + axis) of the nodes this rank owns, ascending."""
        return (3 * self.owned_nodes()[:, None] + np.arange(3)[None, :]).ravel()

    def comm_init(self, rank, nranks, unique_id):
        """unique_id: the 128 bytes rank 0 obtained from comm_unique_id()."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._chk(self._lib.feahip_comm_init(self._ctx, rank, nranks, buf))

    def sync(self):
        self._chk(self._lib.feahip_sync(self._ctx))

    def time_kernel(self, what, warmup=2, iters=10):
        ms = C.c_double(0)
        self._chk(self._lib.feahip_time_kernel(self._ctx, what, warmup, iters, C.byref(ms)))
        return ms.value

    def sizes(self):
        o = (C.c_longlong * 8)()
        self._chk(self._lib.feahip_sizes(self._ctx, o))
        keys = ["N", "E", "npe", "G", "nnzb", "nchunks", "aux_bytes", "max_rowlen"]
        return dict(zip(keys, [int(v) for v in o]))

    def copy_bandwidth(self, nbytes=1 << 30):
        """GB/s of a plain device copy (read + written) on this box."""
        v = C.c_double(0)
        self._chk(self._lib.feahip_copy_bandwidth(self._ctx, nbytes, C.byref(v)))
        return v.value

    def assembly_stats(self):
        """dict: element evaluations per element of the gather chunks, chunks, chunks with their predecessor's map
        words, map bytes (zeros when another strategy runs)."""
        v = (C.c_double * 4)()
        self._chk(self._lib.feahip_assembly_stats(self._ctx, v))
        return {"evals_per_element": float(v[0]), "chunks": int(v[1]), "chunks_with_predecessors_words": int(v[2]), "map_bytes": int(v[3])}

    def copy_bandwidth_detail(self, nbytes=1 << 30):
        """The same four ways: [one 16-byte load in flight per lane, four in flight per lane, hipMemcpyDtoDAsync,
        four in flight non-temporal]."""
        v = (C.c_double * 4)()
        self._chk(self._lib.feahip_copy_bandwidth_detail(self._ctx, nbytes, v))
        return [float(x) for x in v]

    def device_layout(self):
        o = (C.c_longlong * 4)()
        self._chk(self._lib.feahip_device_layout(self._ctx, o))
        return {"K": int(o[0]), "colidx": int(o[1]), "p": int(o[2]), "q": int(o[3])}

    def assembly_in_use(self):
        """The strategy the most recent assembly launch ran (what ASM_AUTO resolved to)."""
        v = C.c_int(0)
        self._chk(self._lib.feahip_assembly_in_use(self._ctx, C.byref(v)))
        return v.value


def host_numbering(elements, nodes):
    """(library id of every node, renumbered?) that feahip_create would choose for this mesh; host only."""
    el = np.ascontiguousarray(elements, dtype=np.int32)
    x = np.ascontiguousarray(nodes, dtype=np.float64)
    out = np.empty(len(x), dtype=np.int32)
    rc = load_library().feahip_host_numbering(len(x), el.shape[0], el.shape[1], _i(el), _d(x), _i(out))
    if rc < 0:
        raise FeaHipError(f"feahip_host_numbering failed ({rc})")
    return out, bool(rc)


def host_surface_faces(elements, n_nodes, faces):
    """(owning element[F], local face[F], index of the first bad face or -1) of the faces, as feahip_set_surface_loads
    resolves them (host only).  Local faces: tetrahedra 0..3 opposite vertex 3, 2, 1, 0; bricks t-, t+, s-, r+, s+, r-."""
    el = np.ascontiguousarray(elements, dtype=np.int32)
    fc = np.ascontiguousarray(faces, dtype=np.int32)
    fc = fc.reshape(len(fc), -1)
    fe, fl = np.full(len(fc), -1, dtype=np.int32), np.full(len(fc), -1, dtype=np.int32)
    bad = C.c_int(-1)
    rc = load_library().feahip_host_surface_faces(n_nodes, el.shape[0], el.shape[1], _i(el), len(fc), fc.shape[1],
                                                  _i(fc), _i(fe), _i(fl), C.byref(bad))
    if rc not in (0, -1):
        raise FeaHipError(f"feahip_host_surface_faces failed ({rc})")
    return fe, fl, int(bad.value)


def host_gather_stats(elements, n_nodes):
    """Shape of the GATHER maps of a mesh (4-, 10- or 8-node elements) in the numbering given (host only): dict + chunks by row count."""
    el = np.ascontiguousarray(elements, dtype=np.int32)
    st = np.zeros(8, dtype=np.int64)
    hist = np.zeros(65, dtype=np.int32)
    rc = load_library().feahip_host_gather_stats(n_nodes, el.shape[0], el.shape[1], _i(el), st.ctypes.data_as(C.POINTER(C.c_longlong)), _i(hist))
    if rc:
        raise FeaHipError(f"feahip_host_gather_stats failed ({rc})")
    return {"chunks": int(st[0]), "evals": int(st[1]), "elements": int(st[2]), "rows": int(st[3]),
            "evals_per_element": float(st[1]) / float(st[2]), "rows_per_chunk": float(st[3]) / float(st[0]),
            "chunks_with_predecessors_words": int(st[4]), "map_bytes": int(st[5]),
            "chunks_with_long_block_lists": int(st[6]), "chunks_with_long_diagonal_lists": int(st[7])}, hist


def host_gather_walk(elements, n_nodes, rows=None, ncu=0):
    """The walk of the 4-node GATHER maps of a mesh in the numbering given (host only), under the FEAHIP_GATHER_ORDER /
    _BALANCE / _RUN / _NRUNS settings of the environment; rows = (first, end) for a rank's rows; ncu: the compute units
    the runs are cut for (0: 256).  dict: walk[i] = the chunk (in row order) whose record is the i-th of the maps,
    run_start[nruns + 1], cost[i] = modelled cycles of record i, blob = the map records (uint8, `stride` bytes each; the
    map words of a record are its bytes [words_begin, words_end)), launch_cost = modelled cycles of a launch."""
    el = np.ascontiguousarray(elements, dtype=np.int32)
    lib = load_library()
    r0, r1 = rows if rows is not None else (0, 0)
    info = np.zeros(8, dtype=np.int64)
    ip = info.ctypes.data_as(C.POINTER(C.c_longlong))
    n = lib.feahip_host_gather_walk(n_nodes, el.shape[0], _i(el), r0, r1, ncu, ip, 0, None, None, None, 0, None)
    if n < 0:
        raise FeaHipError(f"feahip_host_gather_walk failed ({n})")
    walk, start, cost = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    blob = np.zeros(int(info[5]), dtype=np.uint8)
    if lib.feahip_host_gather_walk(n_nodes, el.shape[0], _i(el), r0, r1, ncu, ip, n, _i(walk), _i(start), _i(cost), len(blob),
                                   blob.ctypes.data_as(C.c_void_p)) != n:
        raise FeaHipError("feahip_host_gather_walk: chunk count changed")
    return {"chunks": n, "runs": int(info[1]), "stride": int(info[2]), "words_begin": int(info[3]), "words_end": int(info[4]),
            "chunks_with_predecessors_words": int(info[6]), "launch_cost": int(info[7]), "walk": walk,
            "run_start": start[:int(info[1]) + 1].copy(), "cost": cost, "blob": blob}


def host_gather_chunks(elements, n_nodes):
    """Per chunk of the 4-node GATHER maps, in walk order (host only): int array of flags -- bit 0 the next chunk
    repeats this chunk's map words, bit 1 a block list, bit 2 a diagonal list longer than the registers hold."""
    el = np.ascontiguousarray(elements, dtype=np.int32)
    lib = load_library()
    n = lib.feahip_host_gather_chunks(n_nodes, el.shape[0], _i(el), 0, None)
    if n < 0:
        raise FeaHipError(f"feahip_host_gather_chunks failed ({n})")
    flags = np.zeros(n, dtype=np.int32)
    if lib.feahip_host_gather_chunks(n_nodes, el.shape[0], _i(el), n, _i(flags)) != n:
        raise FeaHipError("feahip_host_gather_chunks: chunk count changed")
    return flags


G10_LIMITS = {0: None, 1: "elements", 2: "row length", 3: "tasks", 4: "residual lanes", 5: "list length", 6: "passes",
              7: "other"}


def host_gather10_shape(elements, n_nodes):
    """The edges the 10-node / 8-node GATHER maps of a mesh reach, in the numbering given (host only; pass library ids,
    host_numbering, to see what a context builds).  FEAHIP_GATHER10_ROWS / _ELEMS / _ALPHA apply as they do there."""
    el = np.ascontiguousarray(elements, dtype=np.int32)
    o = np.zeros(16, dtype=np.int64)
    rc = load_library().feahip_host_gather10_shape(n_nodes, el.shape[0], el.shape[1], _i(el), o.ctypes.data_as(C.POINTER(C.c_longlong)))
    if rc:
        raise FeaHipError(f"feahip_host_gather10_shape failed ({rc})")
    ok = bool(o[0])
    return {"ok": ok, "limit": G10_LIMITS[int(o[1])], "chunks": int(o[2]), "max_elems": int(o[3]), "max_nodes": int(o[4]),
            "max_passes": int(o[5]), "min_passes": int(o[6]) if ok else 0, "longest_list": int(o[7]),
            "chunks_with_long_lists": int(o[8]), "max_fdw": int(o[9]), "tile_blocks": int(o[10]),
            "chunks_at_elem_limit": int(o[11]), "zero_slot": int(o[12]), "first_long_list_chunk": int(o[13]),
            "limit_row": int(o[14]), "max_rows": int(o[15])}


def host_assembly_digest(elements, n_nodes, rank=0, nranks=1):
    """(rowhash[N] uint64, (row0, row1)) of the assembly maps `rank` of `nranks` builds on the host (no device)."""
    el = np.ascontiguousarray(elements, dtype=np.int32)
    h = np.zeros(n_nodes, dtype=np.uint64)
    rows = np.zeros(2, dtype=np.int32)
    rc = load_library().feahip_host_assembly_digest(n_nodes, el.shape[0], el.shape[1], _i(el), rank, nranks,
                                                    h.ctypes.data_as(C.POINTER(C.c_ulonglong)), _i(rows))
    if rc:
        raise FeaHipError(f"feahip_host_assembly_digest failed ({rc})")
    return h, (int(rows[0]), int(rows[1]))


def host_coarse_aggregates(n_owned, m):
    """Host only: the cuts of preconditioner 2's aggregates over n_owned rows under the cap m
    (feahip_host_coarse_aggregates): first rows [m_r + 1], counted from the rank's first owned row."""
    lib = load_library()
    mr = lib.feahip_host_coarse_aggregates(n_owned, m, None)
    if mr < 1:
        raise FeaHipError(f"feahip_host_coarse_aggregates failed ({mr})")
    first = np.zeros(mr + 1, dtype=np.int32)
    lib.feahip_host_coarse_aggregates(n_owned, m, _i(first))
    return first


def comm_unique_id():
    buf = C.create_string_buffer(128)
    n = load_library().feahip_comm_unique_id(buf, 128)
    if n <= 0:
        raise FeaHipError(f"feahip_comm_unique_id failed ({n})")
    return bytes(buf.raw[:128])


def shard_plan(deck, rank, nranks):
    """Host-only halo plan of one rank: dict(row0,row1,peers,send,recv) with
    per-peer node-id arrays."""
    lib = load_library()
    el = np.ascontiguousarray(deck.elements, dtype=np.int32)
    counts = np.zeros(5, dtype=np.int32)
    args = (len(deck.nodes), len(el), el.shape[1], _i(el), rank, nranks)
    rc = lib.feahip_shard_plan(*args, _i(counts), None, None, None, None, None)
    if rc != 0:
        raise FeaHipError(f"feahip_shard_plan failed ({rc})")
    npeer, nsend, nrecv = int(counts[0]), int(counts[1]), int(counts[2])
    peers = np.zeros(max(npeer, 1), dtype=np.int32)
    soff, roff = np.zeros(npeer + 1, dtype=np.int32), np.zeros(npeer + 1, dtype=np.int32)
    sidx, ridx = np.zeros(max(nsend, 1), dtype=np.int32), np.zeros(max(nrecv, 1), dtype=np.int32)
    rc = lib.feahip_shard_plan(*args, _i(counts), _i(peers), _i(soff), _i(roff), _i(sidx), _i(ridx))
    if rc != 0:
        raise FeaHipError(f"feahip_shard_plan failed ({rc})")
    return {"row0": int(counts[3]), "row1": int(counts[4]), "peers": [int(p) for p in peers[:npeer]],
            "send": [sidx[soff[k]:soff[k + 1]].copy() for k in range(npeer)],
            "recv": [ridx[roff[k]:roff[k + 1]].copy() for k in range(npeer)]}


class RankSolver(FeaSolver):
    """One rank's context of a sharded run (feahip_create_rank): the sub-mesh this rank holds, locally indexed (owned
    nodes first).  node_global / elem_global say which nodes and elements of the deck the local ones are; every
    node- or element-indexed method speaks local indices."""

    def __init__(self, deck, rank, nranks, device=0):            # noqa: super().__init__ not called: another constructor of the ABI
        self._lib = load_library()
        self._ctx = C.c_void_p()
        self.deck = deck
        w, _, dforms = element_tables(deck.ele_type, deck.gauss_nodes_count)
        self.npe, self.G = deck.nodes_per_element, deck.gauss_nodes_count
        par = np.zeros(10)
        par[:2] = deck.parameters[:2]
        rc = self._lib.feahip_create_rank(
            C.byref(self._ctx), device, rank, nranks, len(deck.nodes), len(deck.elements), self.npe, self.G, _d(w), _d(dforms),
            _i(deck.elements), _d(deck.nodes), deck.model, _d(par), 2, len(deck.presc_node), _i(deck.presc_node),
            _i(deck.presc_type), _d(deck.presc_values))
        if rc != 0:
            self._ctx = C.c_void_p()
            raise FeaHipError(f"feahip_create_rank failed ({rc}): {self._lib.feahip_create_error().decode()}")
        o = (C.c_longlong * 8)()
        self._chk(self._lib.feahip_rank_counts(self._ctx, o))
        self.N, self.n_own, self.E, self.N_global = int(o[0]), int(o[1]), int(o[2]), int(o[3])
        self.nnzb_local, self.nnzb_owned, self.rows_sent, self.rows_received = int(o[4]), int(o[5]), int(o[6]), int(o[7])
        self.ndof = 3 * self.N
        self.node_global = np.empty(self.N, dtype=np.int32)
        self.elem_global = np.empty(self.E, dtype=np.int32)
        self._chk(self._lib.feahip_rank_maps(self._ctx, _i(self.node_global), _i(self.elem_global)))
        self._deck_surface_loads()                              # the whole face list: the rank keeps what touches its nodes
        self._deck_contact()                                    # the same rule
        self._deck_materials()                                  # the whole mesh's ids: the rank keeps its own elements'
        self._deck_mass()


def host_rank_mesh(deck, rank, nranks, pattern=False):
    """Host only: what rank `rank` of `nranks` would hold.  dict of counts; with pattern=True also node_global, elem_global
    and the block rows of the owned nodes (rowptr, colidx in the deck's node ids)."""
    lib = load_library()
    el = np.ascontiguousarray(deck.elements, dtype=np.int32)
    x = np.ascontiguousarray(deck.nodes, dtype=np.float64)
    cnt = (C.c_longlong * 8)()
    args = (rank, nranks, len(x), el.shape[0], el.shape[1], _i(el), _d(x))
    rc = lib.feahip_host_rank_mesh(*args, cnt, None, None, None, None)
    if rc != 0:
        raise FeaHipError(f"feahip_host_rank_mesh failed ({rc})")
    names = ("local_nodes", "owned_nodes", "local_elements", "blocks_owned_rows", "blocks_local_rows", "peers", "rows_sent", "rows_received")
    out = {k: int(v) for k, v in zip(names, cnt)}
    if pattern:
        ng = np.empty(out["local_nodes"], dtype=np.int32); eg = np.empty(out["local_elements"], dtype=np.int32)
        rp = np.empty(out["owned_nodes"] + 1, dtype=np.int64); ci = np.empty(max(out["blocks_owned_rows"], 1), dtype=np.int32)
        rc = lib.feahip_host_rank_mesh(*args, cnt, _i(ng), _i(eg), rp.ctypes.data_as(C.POINTER(C.c_longlong)), _i(ci))
        if rc != 0:
            raise FeaHipError(f"feahip_host_rank_mesh failed ({rc})")
        out.update(node_global=ng, elem_global=eg, rowptr=rp, colidx=ci[:out["blocks_owned_rows"]])
    return out


def host_rank_plan(deck, rank, nranks):
    """Host only: halo plan of one rank's sub-mesh in the deck's node ids: dict(peers, send, recv)."""
    lib = load_library()
    el = np.ascontiguousarray(deck.elements, dtype=np.int32)
    x = np.ascontiguousarray(deck.nodes, dtype=np.float64)
    cnt = np.zeros(3, dtype=np.int32)
    args = (rank, nranks, len(x), el.shape[0], el.shape[1], _i(el), _d(x))
    if lib.feahip_host_rank_plan(*args, _i(cnt), None, None, None, None, None) != 0:
        raise FeaHipError("feahip_host_rank_plan failed")
    npeer, nsend, nrecv = (int(v) for v in cnt)
    peers = np.zeros(max(npeer, 1), dtype=np.int32)
    soff, roff = np.zeros(npeer + 1, dtype=np.int32), np.zeros(npeer + 1, dtype=np.int32)
    sidx, ridx = np.zeros(max(nsend, 1), dtype=np.int32), np.zeros(max(nrecv, 1), dtype=np.int32)
    if lib.feahip_host_rank_plan(*args, _i(cnt), _i(peers), _i(soff), _i(roff), _i(sidx), _i(ridx)) != 0:
        raise FeaHipError("feahip_host_rank_plan failed")
    return {"peers": [int(p) for p in peers[:npeer]],
            "send": [sidx[soff[k]:soff[k + 1]].copy() for k in range(npeer)],
            "recv": [ridx[roff[k]:roff[k + 1]].copy() for k in range(npeer)]}


class Slab:
    """What ONE rank of a run holds when the caller partitions the mesh itself (feahip_create_rank_local): local nodes
    -- [0, n_own) owned, then the halo nodes of the elements around them -- those elements in LOCAL node ids, the global
    id of every local node and element, the owner of every halo node, the prescribed entries of every local node (halo
    nodes included) and optional surface faces, both in local ids.  Material, element and solver fields as Deck."""

    def __init__(self, **kw):
        self.model = kw.get("model", MODEL_COMPRESSIBLE_NEOHOOKEAN)
        self.parameters = np.array(kw.get("parameters", [100.0, 100.0]), dtype=np.float64)
        self.solver_type = kw.get("solver_type", CG)
        self.solver_tolerance = kw.get("solver_tolerance", 1e-14)
        self.solver_max_iter = kw.get("solver_max_iter", 20000)
        self.ele_type = kw.get("ele_type", TETRAHEDRA10)
        self.load_increments_count = kw.get("load_increments_count", 1)
        self.desired_tolerance = kw.get("desired_tolerance", 1e-8)
        self.max_newton_count = kw.get("max_newton_count", 20)
        self.modified_newton = kw.get("modified_newton", True)
        self.gauss_nodes_count = kw.get("gauss_nodes_count", 5)
        self.nodes = np.ascontiguousarray(kw["nodes"], dtype=np.float64).reshape(-1, 3)
        self.elements = np.ascontiguousarray(kw["elements"], dtype=np.int32)
        self.nodes_per_element = self.elements.shape[1]
        self.node_global = np.ascontiguousarray(kw["node_global"], dtype=np.int32)
        eg = kw.get("elem_global")
        self.elem_global = np.arange(len(self.elements), dtype=np.int32) if eg is None else np.ascontiguousarray(eg, dtype=np.int32)
        self.n_own = int(kw["n_own"])
        self.n_global_nodes = int(kw["n_global_nodes"])
        self.halo_owner = np.ascontiguousarray(kw.get("halo_owner", []), dtype=np.int32)
        self.presc_node = np.ascontiguousarray(kw.get("presc_node", []), dtype=np.int32)
        self.presc_type = np.ascontiguousarray(kw.get("presc_type", []), dtype=np.int32)
        self.presc_values = np.ascontiguousarray(kw.get("presc_values", np.zeros((0, 3))), dtype=np.float64).reshape(-1, 3)
        faces = np.asarray(kw.get("surface_faces", np.zeros((0, 0))), dtype=np.int32)
        self.surface_faces = np.ascontiguousarray(faces.reshape(len(faces), -1) if faces.size else np.zeros((0, 0), dtype=np.int32))
        self.surface_kind = np.ascontiguousarray(kw.get("surface_kind", []), dtype=np.int32)
        self.surface_values = np.ascontiguousarray(kw.get("surface_values", np.zeros((0, 3))), dtype=np.float64).reshape(-1, 3)
        _take_contact(self, kw)
        # material table (feahip_set_materials): materials[n][2] = lambda, mu and one id per element; none = the single
        # pair `parameters`
        self.materials = np.ascontiguousarray(kw.get("materials", np.zeros((0, 2))), dtype=np.float64).reshape(-1, 2)
        self.element_material = np.ascontiguousarray(kw.get("element_material", []), dtype=np.int32)
        if len(self.element_material) != (len(self.elements) if len(self.materials) else 0):
            raise ValueError("materials and element_material come together, one id per element")
        _take_dynamics(self, kw)

    def permuted(self, new_local_id):
        """The same slab with local node a renamed new_local_id[a] (owned ids must stay in [0, n_own))."""
        import copy
        new = np.ascontiguousarray(new_local_id, dtype=np.int32)
        n, no = len(self.nodes), self.n_own
        if not (np.array_equal(np.sort(new), np.arange(n)) and np.all(new[:no] < no)):
            raise ValueError("not a permutation of the local ids that keeps the owned nodes first")
        out = copy.copy(self)
        out.nodes = np.empty_like(self.nodes); out.nodes[new] = self.nodes
        out.node_global = np.empty_like(self.node_global); out.node_global[new] = self.node_global
        out.halo_owner = np.empty_like(self.halo_owner); out.halo_owner[new[no:] - no] = self.halo_owner
        out.elements = np.ascontiguousarray(new[self.elements])
        out.presc_node = np.ascontiguousarray(new[self.presc_node]) if len(self.presc_node) else self.presc_node
        if len(self.surface_kind):
            out.surface_faces = np.ascontiguousarray(new[self.surface_faces])
        if len(self.contact_faces):
            out.contact_faces = np.ascontiguousarray(new[self.contact_faces])
        return out

    def reordered(self):
        """The slab in the local order feahip_host_slab_order proposes: the library's numbering of the local mesh,
        owned nodes first."""
        new = np.empty(len(self.nodes), dtype=np.int32)
        rc = load_library().feahip_host_slab_order(len(self.nodes), self.n_own, len(self.elements), self.nodes_per_element,
                                                   _i(self.elements), _d(self.nodes), _i(new))
        if rc < 0:
            raise FeaHipError(f"feahip_host_slab_order failed ({rc})")
        return self.permuted(new) if rc else self


class LocalRankSolver(FeaSolver):
    """One rank's context from its own slab (feahip_create_rank_local): what RankSolver is, made without the whole mesh.
    Every node- or element-indexed method speaks the slab's local indices; surface faces are local too."""

    def __init__(self, slab, rank, nranks, device=0):            # noqa: super().__init__ not called: another constructor of the ABI
        self._lib = load_library()
        self._ctx = C.c_void_p()
        self.deck = self.slab = slab
        w, _, dforms = element_tables(slab.ele_type, slab.gauss_nodes_count)
        self.npe, self.G = slab.nodes_per_element, slab.gauss_nodes_count
        par = np.zeros(10)
        par[:2] = slab.parameters[:2]
        rc = self._lib.feahip_create_rank_local(
            C.byref(self._ctx), device, rank, nranks, slab.n_global_nodes, len(slab.nodes), slab.n_own, len(slab.elements),
            self.npe, self.G, _d(w), _d(dforms), _i(slab.elements), _d(slab.nodes), _i(slab.node_global), _i(slab.elem_global),
            _i(slab.halo_owner), slab.model, _d(par), 2, len(slab.presc_node), _i(slab.presc_node), _i(slab.presc_type),
            _d(slab.presc_values))
        if rc != 0:
            self._ctx = C.c_void_p()
            raise FeaHipError(f"feahip_create_rank_local failed ({rc}): {self._lib.feahip_create_error().decode()}")
        o = (C.c_longlong * 8)()
        self._chk(self._lib.feahip_rank_counts(self._ctx, o))
        self.N, self.n_own, self.E, self.N_global = int(o[0]), int(o[1]), int(o[2]), int(o[3])
        self.nnzb_local, self.nnzb_owned, self.rows_sent, self.rows_received = int(o[4]), int(o[5]), int(o[6]), int(o[7])
        self.ndof = 3 * self.N
        self.node_global = np.empty(self.N, dtype=np.int32)
        self.elem_global = np.empty(self.E, dtype=np.int32)
        self._chk(self._lib.feahip_rank_maps(self._ctx, _i(self.node_global), _i(self.elem_global)))
        self._deck_surface_loads()                              # local ids; faces of other ranks' nodes are dropped
        self._deck_contact()
        self._deck_materials()                                  # the slab's own ids, in its element order
        self._deck_mass()


def host_rank_local_plan(slab, rank, nranks):
    """Host only: the halo plan feahip_create_rank_local installs for this slab, in GLOBAL node ids:
    dict(peers, send, recv), rows ascending in global id inside every peer."""
    lib = load_library()
    cnt = np.zeros(3, dtype=np.int32)
    args = (rank, nranks, len(slab.nodes), slab.n_own, len(slab.elements), slab.nodes_per_element, _i(slab.elements),
            _i(slab.node_global), _i(slab.halo_owner))
    rc = lib.feahip_host_rank_local_plan(*args, _i(cnt), None, None, None, None, None)
    if rc != 0:
        raise FeaHipError(f"feahip_host_rank_local_plan failed ({rc}): {lib.feahip_create_error().decode()}")
    npeer, nsend, nrecv = (int(v) for v in cnt)
    peers = np.zeros(max(npeer, 1), dtype=np.int32)
    soff, roff = np.zeros(npeer + 1, dtype=np.int32), np.zeros(npeer + 1, dtype=np.int32)
    sidx, ridx = np.zeros(max(nsend, 1), dtype=np.int32), np.zeros(max(nrecv, 1), dtype=np.int32)
    rc = lib.feahip_host_rank_local_plan(*args, _i(cnt), _i(peers), _i(soff), _i(roff), _i(sidx), _i(ridx))
    if rc != 0:
        raise FeaHipError(f"feahip_host_rank_local_plan failed ({rc}): {lib.feahip_create_error().decode()}")
    return {"peers": [int(p) for p in peers[:npeer]],
            "send": [sidx[soff[k]:soff[k + 1]].copy() for k in range(npeer)],
            "recv": [ridx[roff[k]:roff[k + 1]].copy() for k in range(npeer)]}


def slab_of(deck, rank, nranks):
    """Cuts a whole deck into the Slab of one rank, with the library's own cut and local order (host_rank_mesh): the
    slab RankSolver(deck, rank, nranks) holds.  A bridge for callers that still have the whole deck, and for tests."""
    N = len(deck.nodes)
    meshes = [host_rank_mesh(deck, r, nranks, pattern=True) for r in range(nranks)]
    owner = np.full(N, -1, dtype=np.int32)
    for r, m in enumerate(meshes):
        owner[m["node_global"][:m["owned_nodes"]]] = r
    m = meshes[rank]
    ng, eg, no = m["node_global"], m["elem_global"], m["owned_nodes"]
    local_of = np.full(N, -1, dtype=np.int64)
    local_of[ng] = np.arange(len(ng))
    kw = {k: getattr(deck, k) for k in ("model", "parameters", "solver_type", "solver_tolerance", "solver_max_iter", "ele_type",
                                         "load_increments_count", "desired_tolerance", "max_newton_count", "modified_newton",
                                         "gauss_nodes_count")}
    keep = local_of[deck.presc_node] >= 0 if len(deck.presc_node) else np.zeros(0, dtype=bool)
    if len(getattr(deck, "surface_kind", [])):
        fl = local_of[deck.surface_faces]
        fk = np.all(fl >= 0, axis=1)                            # all of its nodes are local (the library drops other ranks')
        kw.update(surface_faces=fl[fk], surface_kind=deck.surface_kind[fk], surface_values=deck.surface_values[fk])
    if len(getattr(deck, "contact_faces", [])) and len(deck.contact_obstacles):
        fl = local_of[deck.contact_faces]
        kw.update(contact_faces=fl[np.all(fl >= 0, axis=1)], contact_obstacles=deck.contact_obstacles,
                  contact_penalty=deck.contact_penalty, contact_augment=deck.contact_augment,
                  contact_gap_tolerance=deck.contact_gap_tolerance)
    if len(getattr(deck, "materials", [])):
        kw.update(materials=deck.materials, element_material=deck.element_material[eg])
    slab = Slab(nodes=deck.nodes[ng], elements=local_of[deck.elements[eg]], node_global=ng, elem_global=eg, n_own=no,
                n_global_nodes=N, halo_owner=owner[ng[no:]], presc_node=local_of[deck.presc_node[keep]] if keep.any() else [],
                presc_type=deck.presc_type[keep] if keep.any() else [],
                presc_values=deck.presc_values[keep] if keep.any() else np.zeros((0, 3)), **kw)
    for k in ("linesearch_max", "arclength_max", "density", "body_force", "dynamics", "damping"):
        if hasattr(deck, k):
            setattr(slab, k, getattr(deck, k))
    return slab


class FeaGroup:
    """n contexts of one mesh sharded by rows and driven from this process
    (feahip_group_* entries)."""

    def __init__(self, deck, n=None, device=0, rank_contexts=False):
        """rank_contexts: every rank holds only its sub-mesh (RankSolver) instead of the whole mesh with a row shard.
        deck may be a list of Slabs, one per rank: every rank is made from its own slab (LocalRankSolver)."""
        slabs = list(deck) if isinstance(deck, (list, tuple)) else None
        if slabs is not None:
            if n not in (None, len(slabs)):
                raise ValueError("n slabs make n ranks")
            n, rank_contexts = len(slabs), True
        self.deck, self.n = deck, n
        self.n_global = slabs[0].n_global_nodes if slabs is not None else len(deck.nodes)
        self.rank_contexts = rank_contexts
        if slabs is not None:
            self.ranks = [LocalRankSolver(s, r, n, device=device) for r, s in enumerate(slabs)]
        elif rank_contexts:
            self.ranks = [RankSolver(deck, r, n, device=device) for r in range(n)]
        else:
            self.ranks = [FeaSolver(deck, device=device) for _ in range(n)]
        self._lib = load_library()
        self._arr = (C.c_void_p * n)(*[r._ctx for r in self.ranks])
        self._chk(self._lib.feahip_group_init(self._arr, n))
        dm = getattr(slabs[0] if slabs is not None else deck, "damping", None)
        if dm is not None and dm[1] > 0.0:                      # K_d is keyed by the row shard, which the line above installed
            self.set_damping(*dm)
        self.rows = [r.owned_rows() for r in self.ranks]        # library ids (local ids for rank contexts)
        if rank_contexts:
            self.nodes = [r.node_global[:r.n_own].astype(np.int64) for r in self.ranks]
        else:
            self.nodes = [r.owned_nodes() for r in self.ranks]  # the caller's ids of every rank's nodes

    def _chk(self, rc):
        if rc != 0:
            msgs = [self._lib.feahip_last_error(r._ctx).decode() for r in self.ranks]
            raise FeaHipError(f"libfeahip group error {rc}: {msgs}")

    def each(self, name, *args):
        return [getattr(r, name)(*args) for r in self.ranks]

    def apply_preconditioner(self, r):
        """Every rank's z = M^-1 r on its own rows, stitched together: the preconditioner the group's PCG uses
        (block-diagonal over the ranks for kinds 0 and 1).  r in the deck's node ids."""
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1, 3)
        z = np.zeros_like(r)
        if all(getattr(rk, "preconditioner", 0) == 2 for rk in self.ranks):
            # the coarse level spans the ranks: one collective application (feahip_group_apply_preconditioner)
            rs = [np.ascontiguousarray(r[rk.node_global] if self.rank_contexts else r).ravel() for rk in self.ranks]
            zs = [np.zeros(rk.ndof) for rk in self.ranks]
            rp, zp = (_dp * self.n)(*[_d(v) for v in rs]), (_dp * self.n)(*[_d(v) for v in zs])
            self._chk(self._lib.feahip_group_apply_preconditioner(self._arr, self.n, rp, zp))
            for rk, nd, zr in zip(self.ranks, self.nodes, zs):
                z[nd] += zr.reshape(-1, 3)[:rk.n_own] if self.rank_contexts else zr.reshape(-1, 3)[nd]
            return z.ravel()
        for rk, nd in zip(self.ranks, self.nodes):
            if self.rank_contexts:
                zr = rk.apply_preconditioner(r[rk.node_global]).reshape(-1, 3)
                z[nd] += zr[:rk.n_own]
            else:
                z[nd] += rk.apply_preconditioner(r).reshape(-1, 3)[nd]
        return z.ravel()

    def amg_info(self):
        return self.each("amg_info")

    def amg_level(self, level):
        return self.each("amg_level", level)

    def solve_slae(self, solver_type, tolerance, max_iterations):
        it, res = C.c_int(0), C.c_double(0)
        self._chk(self._lib.feahip_group_solve_slae(self._arr, self.n, solver_type, tolerance, max_iterations,
                                                    C.byref(it), C.byref(res)))
        return it.value, res.value

    def energy(self):
        t = C.c_double(0)
        self._chk(self._lib.feahip_group_energy(self._arr, self.n, C.byref(t)))
        return t.value

    def update_nodes_with_solution(self):
        self._chk(self._lib.feahip_group_update_nodes_with_solution(self._arr, self.n))

    def solve(self, load_increments, max_newton, modified_newton, desired_tolerance, solver_type,
              solver_tolerance=1e-14, solver_max_iter=20000):
        cap = load_increments * max_newton
        tol_log = np.zeros(cap)
        its = np.zeros(load_increments, dtype=np.int32)
        done = C.c_int(0)
        self._chk(self._lib.feahip_group_solve(self._arr, self.n, load_increments, max_newton, int(modified_newton),
                                               desired_tolerance, solver_type, solver_tolerance, solver_max_iter,
                                               _d(tol_log), cap, _i(its), C.byref(done)))
        return done.value, its, tol_log[:int(its.sum())]

    def set_mass(self, rho):
        self.each("set_mass", rho)

    def set_body_force(self, b):
        self.each("set_body_force", b)

    def set_damping(self, alpha, beta=0.0):
        """Every member takes the snapshot of its own rows (the call is per context)."""
        self.each("set_damping", alpha, beta)

    def consistent_acceleration(self, solver_type, tolerance=1e-14, max_iterations=20000):
        self.ranks[0].consistent_acceleration(solver_type, tolerance, max_iterations)   # one call drives the group

    def solve_dynamic(self, n_steps, dt, beta, gamma, dlambda, max_newton, desired_tolerance, solver_type,
                      solver_tolerance=1e-14, solver_max_iter=20000):
        cap = max(n_steps * max_newton, 1)
        tol_log, its, done = np.zeros(cap), np.zeros(max(n_steps, 1), dtype=np.int32), C.c_int(0)
        self._chk(self._lib.feahip_group_solve_dynamic(self._arr, self.n, n_steps, dt, beta, gamma, dlambda, max_newton,
                                                       desired_tolerance, solver_type, solver_tolerance, solver_max_iter,
                                                       _d(tol_log), cap, _i(its), C.byref(done)))
        n = int(its[:min(done.value + 1, n_steps)].sum())
        return done.value, its[:n_steps], tol_log[:n]

    def stable_step(self):
        return self.ranks[0].stable_step()                      # one call drives the group

    def kinetic_energy(self):
        return self.ranks[0].kinetic_energy()

    def strain_energy(self):
        return self.ranks[0].strain_energy()                    # one call drives the group

    def contact_info(self):
        return self.ranks[0].contact_info()

    def contact_augment(self):
        return self.ranks[0].contact_augment()

    # ---- modal analysis over the ranks -------------------------------------
    def solve_modes(self, n_modes, tolerance=1e-8, max_iterations=1000, warm=False, check=True):
        """feahip_solve_modes_sharded on the group (one call drives it): (lam[n_modes], resid[n_modes], steps) and, with
        check=False, the return code as a fourth item instead of raising when the steps run out."""
        lam, res, it = np.zeros(max(int(n_modes), 1)), np.zeros(max(int(n_modes), 1)), C.c_int(0)
        rc = self._lib.feahip_solve_modes_sharded(self.ranks[0]._ctx, int(n_modes), float(tolerance), int(max_iterations),
                                                  int(bool(warm)), _d(lam), _d(res), C.byref(it))
        if check or rc != ENOTCONVERGED:
            self._chk(rc)
        return (lam, res, it.value) if check else (lam, res, it.value, rc)

    def _stitch_dofs(self, parts):
        """Owned rows of per-rank block arrays [k][3 N_rank], stitched into [k][3 N_global] in the deck's dof order."""
        out = np.zeros((parts[0].shape[0], self.n_global, 3))
        for r, nd, p in zip(self.ranks, self.nodes, parts):
            p = p.reshape(len(p), -1, 3)
            out[:, nd] = p[:, :r.n_own] if self.rank_contexts else p[:, nd]
        return out.reshape(len(out), -1)

    def modes(self, first=0, count=None):
        """The modes of the last solve_modes: every rank's own rows stitched into phi[count][3 N_global] in the deck's
        dof order."""
        return self._stitch_dofs([r.modes(first, count) for r in self.ranks])

    def spmm_km(self, x8, per_rank=False):
        """[K X, mask(M X)] of eight whole-mesh columns x8[8][3 N_global] by the sharded block product
        (feahip_group_spmm_km): every rank multiplies its own rows, the halo rows of X travel by the block exchange.
        per_rank: also every rank's own [8][3 N_rank] results as the library returned them (zero off its rows)."""
        x8 = np.ascontiguousarray(x8, dtype=np.float64).reshape(MODAL_COLS, self.n_global, 3)
        xs = [np.ascontiguousarray(x8[:, r.node_global] if self.rank_contexts else x8).reshape(MODAL_COLS, -1) for r in self.ranks]
        ys, zs = [np.zeros_like(x) for x in xs], [np.zeros_like(x) for x in xs]
        xp, yp, zp = ((_dp * self.n)(*[_d(v) for v in vs]) for vs in (xs, ys, zs))
        self._chk(self._lib.feahip_group_spmm_km(self._arr, self.n, xp, yp, zp))
        out = (self._stitch_dofs(ys), self._stitch_dofs(zs))
        return out + (ys, zs) if per_rank else out

    def _stitch_rows(self, parts):
        """Owned rows of per-node arrays ([N] or [N][k]), stitched together."""
        out = np.zeros((self.n_global,) + parts[0].shape[1:])
        for r, nd, p in zip(self.ranks, self.nodes, parts):
            out[nd] = p[:r.n_own] if self.rank_contexts else p[nd]
        return out

    def lumped_mass(self):
        """The owned rows of every rank's lumped mass, stitched together ([N] of the whole mesh)."""
        out = np.zeros(self.n_global)
        for r, nd in zip(self.ranks, self.nodes):
            ml = r.lumped_mass()
            out[nd] = ml[:r.n_own] if self.rank_contexts else ml[nd]
        return out

    def solve_explicit(self, n_steps, dt, safety=0.9, restep=0, dlambda=0.0):
        log, done = np.zeros(max(n_steps, 1)), C.c_int(0)
        self._chk(self._lib.feahip_group_solve_explicit(self._arr, self.n, n_steps, float(dt), float(safety), int(restep),
                                                        float(dlambda), _d(log), len(log), C.byref(done)))
        return done.value, log[:done.value]

    def gather(self, name):
        """Owned rows of a per-node ([N][3]) or per-dof ([3N]) getter, stitched together."""
        parts = self.each(name)
        if name == "nodal_stresses":                            # (sig6, von_mises, weight): one row per node each
            return tuple(self._stitch_rows([p[k] for p in parts]) for k in range(3))
        if name == "nodal_energy":
            return self._stitch_rows(parts)
        if self.rank_contexts:                                  # local arrays: owned rows are the first n_own
            first = parts[0]
            out = np.zeros((self.n_global, 3)) if first.ndim == 2 else np.zeros(3 * self.n_global)
            for r, p in zip(self.ranks, parts):
                nd = r.node_global[:r.n_own].astype(np.int64)
                if out.ndim == 2:
                    out[nd] = p[:r.n_own]
                else:
                    out.reshape(-1, 3)[nd] = p.reshape(-1, 3)[:r.n_own]
            return out
        out = parts[0].copy()
        for nd, p in zip(self.nodes, parts):
            if out.ndim == 2:
                out[nd] = p[nd]
            else:
                d = (3 * nd[:, None] + np.arange(3)[None, :]).ravel()
                out[d] = p[d]
        return out

    def close(self):
        for r in self.ranks:
            r.close()
