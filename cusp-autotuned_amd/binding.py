"""ctypes binding of include/cusp_mi355x.h.  Plumbing only: every function here forwards to the
C-ABI symbol of the same name with raw device pointers taken from torch tensors.  No compute
happens in Python and nothing falls back to the CPU."""
import ctypes
import os
import subprocess
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "lib", "libcusp_mi355x.so")
_lib = None

FORMAT_CSR, FORMAT_ELL, FORMAT_DIA, FORMAT_COO, FORMAT_HYB = 0, 1, 2, 3, 4
TABLE_COO_SORTED = 5  # tuning-table key only: the launch shape of a COO multiply whose plan found the entries row-sorted
F64, F32 = 0, 1
KERNEL_AUTO = 0
CSR_SCALAR, CSR_VECTOR, CSR_STREAM, CSR_STREAM_PIPE, CSR_BALANCED, CSR_STREAM_C16, CSR_STREAM_WAVE, CSR_STREAM_WAVEV, CSR_STREAM_WAVEX = 1, 2, 3, 4, 5, 6, 7, 8, 9
CSR_STREAM_WAVER, CSR_STREAM_PACKED = 11, 12  # round 4: run-compressed column copy on wave tiles; ... with the values packed beside it (opt-in)
POLICY_COLS16 = 8  # Config.nontemporal bit: CSR_STREAM_WAVEV reads the plan's 16-bit column copy (Plan.csr; in plan.config() only when granted)
ELL_ROW, DIA_ROW, COO_SEGMENTED, COO_LANE4, COO_TILE = 10, 20, 30, 31, 32
CSR_SPMM_ROWS, CSR_SPMM_COLS = 40, 41  # cmi_spmm_csr_*: lane groups per row (row-major blocks) / one lane per row (column-major)


class CmiError(RuntimeError):
    """A non-zero cmi_status (the C++ layer turns the same codes into cusp exceptions)."""

    def __init__(self, status, message):
        super().__init__(f"{message}")
        self.status = status


class Config(ctypes.Structure):
    """struct cmi_config: kernel variant + launch shape (0 = let the tuning table decide)."""
    _fields_ = [
        ("kernel", c_int32), ("block_size", c_int32), ("threads_per_row", c_int32),
        ("rows_per_block", c_int32), ("items_per_thread", c_int32), ("nontemporal", c_int32),
        ("xcd_swizzle", c_int32), ("blocks_per_cu", c_int32),
    ]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}

    def __repr__(self):
        return "Config(" + ", ".join(f"{k}={v}" for k, v in self.as_dict().items()) + ")"


class WaverRule(ctypes.Structure):
    """struct cmi_waver_rule: csr_waver's launch shape and AUTO gates (tuning table "waver_rule")."""
    _fields_ = [
        ("items_per_thread", c_int32), ("cap", c_int32), ("xcd_swizzle", c_int32), ("reserved", c_int32),
        ("min_piece", c_double), ("min_entries", c_int64),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}

    def __repr__(self):
        return "WaverRule(" + ", ".join(f"{k}={v}" for k, v in self.as_dict().items()) + ")"


def lib_path():
    return _LIB_PATH


def build(verbose=False):
    """Compile the HIP library for gfx950 in-tree (make -C csrc).  hipcc cross-compiles without a GPU."""
    out = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j8"], capture_output=True, text=True)
    if verbose or out.returncode != 0:
        print(out.stdout)
        print(out.stderr)
    if out.returncode != 0:
        raise RuntimeError("building libcusp_mi355x.so failed")
    return _LIB_PATH


_PI32 = POINTER(c_int32)


def _declare(L):
    vp, i64, i32 = c_void_p, c_int64, c_int
    cfgp = POINTER(Config)
    L.cmi_status_string.restype = c_char_p
    L.cmi_status_string.argtypes = [c_int]
    L.cmi_last_error.restype = c_char_p
    L.cmi_version.restype = c_int
    L.cmi_device_count.argtypes = [POINTER(c_int)]
    L.cmi_set_device.argtypes = [c_int]
    L.cmi_get_device.argtypes = [POINTER(c_int)]
    L.cmi_device_info.argtypes = [c_int, c_char_p, c_size_t, POINTER(c_int), POINTER(c_int64)]
    L.cmi_malloc.argtypes = [POINTER(c_void_p), c_size_t]
    L.cmi_free.argtypes = [vp]
    for n in ("cmi_memcpy_h2d", "cmi_memcpy_d2h", "cmi_memcpy_d2d"):
        getattr(L, n).argtypes = [vp, vp, c_size_t, vp]
    L.cmi_memset.argtypes = [vp, c_int, c_size_t, vp]
    L.cmi_stream_create.argtypes = [POINTER(c_void_p)]
    L.cmi_stream_destroy.argtypes = [vp]
    L.cmi_stream_synchronize.argtypes = [vp]
    L.cmi_event_create.argtypes = [POINTER(c_void_p)]
    L.cmi_event_destroy.argtypes = [vp]
    L.cmi_event_record.argtypes = [vp, vp]
    L.cmi_event_elapsed_ms.argtypes = [vp, vp, POINTER(c_float)]
    L.cmi_event_synchronize.argtypes = [vp]
    L.cmi_malloc_host.argtypes = [POINTER(c_void_p), c_size_t]
    L.cmi_free_host.argtypes = [vp]
    L.cmi_memcpy_d2h_async.argtypes = [vp, vp, c_size_t, vp]
    L.cmi_device_can_access_peer.argtypes = [c_int, c_int, POINTER(c_int)]
    L.cmi_ipc_get_handle.argtypes = [vp, vp]
    L.cmi_ipc_open_handle.argtypes = [vp, POINTER(c_void_p)]
    L.cmi_ipc_close_handle.argtypes = [vp]
    L.cmi_copy_ranges.argtypes = [c_int, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int64), vp]
    L.cmi_spmv_csr_dot_f64.argtypes = [i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, cfgp, vp]
    for suf in ("f64", "f32"):
        getattr(L, f"cmi_spmv_ell_dot_{suf}").argtypes = [i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, cfgp, vp]
        getattr(L, f"cmi_spmv_dia_dot_{suf}").argtypes = [i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, cfgp, vp]
    L.cmi_tuning_load.argtypes = [c_char_p]
    L.cmi_tuning_save.argtypes = [c_char_p]
    L.cmi_tuning_set.argtypes = [c_int, c_int, c_double, cfgp]
    L.cmi_tuning_select.argtypes = [c_int, c_int, i64, i64, i64, cfgp]
    for suf in ("f64", "f32"):
        getattr(L, f"cmi_spmv_csr_{suf}").argtypes = [i64, i64, i64, vp, vp, vp, vp, vp, i32, cfgp, vp]
        getattr(L, f"cmi_spmm_csr_{suf}").argtypes = [i64, i64, i64, vp, vp, vp, i64, vp, i64, i64, vp, i64, i64, i32, cfgp, vp]
        getattr(L, f"cmi_spmv_coo_{suf}").argtypes = [i64, i64, i64, vp, vp, vp, vp, vp, i32, cfgp, vp]
        sc = c_double if suf == "f64" else c_float  # the fused sweeps take their scalars by value, in T
        getattr(L, f"cmi_spmv_csr_axpby_{suf}").argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, sc, sc, vp, vp, vp]
        getattr(L, f"cmi_csr_jacobi_sweep_{suf}").argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, vp, sc, vp, vp]
        getattr(L, f"cmi_relax_jacobi_update_{suf}").argtypes = [i64, vp, vp, vp, sc, vp, vp]
        getattr(L, f"cmi_csr_gauss_seidel_colour_{suf}").argtypes = [i64, i64, vp, vp, vp, vp, vp, vp, i64, i64, vp, vp]
        getattr(L, f"cmi_spmv_ell_{suf}").argtypes = [i64, i64, i64, i64, vp, vp, vp, vp, vp, i32, cfgp, vp]
        getattr(L, f"cmi_spmv_dia_{suf}").argtypes = [i64, i64, i64, i64, vp, vp, vp, vp, i32, cfgp, vp]
        getattr(L, f"cmi_spmv_hyb_{suf}").argtypes = [i64, i64, i64, i64, vp, vp, i64, vp, vp, vp, vp, vp, i32,
                                                     cfgp, cfgp, vp]
        getattr(L, f"cmi_poisson5pt_csr_{suf}").argtypes = [i64, i64, i64, i64, vp, vp, vp, vp]
        getattr(L, f"cmi_poisson5pt_dia_{suf}").argtypes = [i64, i64, i64, vp, vp, vp]
        getattr(L, f"cmi_csr_to_ell_{suf}").argtypes = [i64, vp, vp, vp, i64, i64, vp, vp, vp]
        getattr(L, f"cmi_csr_to_hyb_coo_{suf}").argtypes = [i64, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    L.cmi_poisson5pt_num_entries.restype = c_int64
    L.cmi_poisson5pt_num_entries.argtypes = [i64, i64]
    L.cmi_poisson5pt_shard_entries.restype = c_int64
    L.cmi_poisson5pt_shard_entries.argtypes = [i64, i64, i64, i64]
    L.cmi_csr_row_indices.argtypes = [i64, vp, vp, vp]
    L.cmi_coo_row_offsets.argtypes = [i64, i64, vp, vp, POINTER(ctypes.c_int), vp]
    L.cmi_csr_interior_rows.argtypes = [i64, vp, vp, i64, i64, POINTER(c_int64), POINTER(c_int64), vp]
    L.cmi_stream_wait_event.argtypes = [vp, vp]
    L.cmi_coo_sort_by_row_f64.argtypes = [i64, i64, i64, vp, vp, vp, ctypes.c_int, vp]
    L.cmi_coo_sort_by_row_f32.argtypes = [i64, i64, i64, vp, vp, vp, ctypes.c_int, vp]
    L.cmi_coo_is_sorted.argtypes = [i64, i64, vp, vp, ctypes.c_int, POINTER(ctypes.c_int), vp]
    for sfx in ("f64", "f32"):
        getattr(L, "cmi_ell_to_csr_" + sfx).argtypes = [i64, i64, i64, vp, vp, vp, vp, vp, i64, POINTER(c_int64), vp]
        getattr(L, "cmi_dia_to_csr_" + sfx).argtypes = [i64, i64, i64, i64, vp, vp, vp, vp, vp, i64, POINTER(c_int64), vp]
        getattr(L, "cmi_hyb_to_csr_" + sfx).argtypes = [i64, i64, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, POINTER(c_int64), vp]
    L.cmi_csr_max_row_length.argtypes = [i64, vp, POINTER(c_int64), vp]
    L.cmi_csr_diagonals.argtypes = [i64, i64, vp, vp, vp, vp, i64, POINTER(c_int64), vp]
    for suf in ("f64", "f32"):
        getattr(L, f"cmi_csr_to_dia_{suf}").argtypes = [i64, i64, vp, vp, vp, i64, i64, vp, vp, vp, vp]
    L.cmi_ell_row_lengths.argtypes = [i64, i64, i64, vp, vp, vp]
    L.cmi_blas_workspace_bytes.restype = c_size_t
    for suf, sc in (("f64", c_double), ("f32", c_float)):
        getattr(L, f"cmi_blas_axpy_{suf}").argtypes = [i64, sc, vp, vp, vp]
        getattr(L, f"cmi_blas_axpby_{suf}").argtypes = [i64, sc, vp, sc, vp, vp, vp]
        getattr(L, f"cmi_blas_copy_{suf}").argtypes = [i64, vp, vp, vp]
        getattr(L, f"cmi_blas_fill_{suf}").argtypes = [i64, sc, vp, vp]
        getattr(L, f"cmi_blas_dot_{suf}").argtypes = [i64, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_blas_nrm2_{suf}").argtypes = [i64, vp, vp, vp, vp]
    for suf in ("f64", "f32"):
        getattr(L, f"cmi_spmv_csr_dot_plan_partials_{suf}").argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, POINTER(c_int), vp]
        getattr(L, f"cmi_cg_update_fold_{suf}").argtypes = [i64, vp, vp, c_int, vp, vp, vp, POINTER(c_int), vp]
        getattr(L, f"cmi_cg_direction_x_fold_{suf}").argtypes = [i64, vp, vp, c_int, vp, vp, vp, vp, vp, vp, vp]
    L.cmi_cg_update_f64.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.cmi_cg_direction_f64.argtypes = [i64, vp, vp, vp, vp, vp]
    L.cmi_cg_direction_x_f64.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp]
    L.cmi_cg_update_f32.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.cmi_cg_direction_f32.argtypes = [i64, vp, vp, vp, vp, vp]
    L.cmi_cg_direction_x_f32.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp]
    L.cmi_blas_dotd_f32.argtypes = [i64, vp, vp, vp, vp, vp]
    for suf, sc in (("f64", c_double), ("f32", c_float)):   # the multi-shift solver steps (csrc/krylov_m.hip)
        getattr(L, f"cmi_cg_m_coefficients_{suf}").argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_cg_m_update_xp_{suf}").argtypes = [i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_bicgstab_m_s_{suf}").argtypes = [i64, sc, sc, vp, vp, vp, vp]
        getattr(L, f"cmi_bicgstab_m_coefficients_{suf}").argtypes = [i64, sc, sc, sc, sc, sc, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_bicgstab_m_update_xs_{suf}").argtypes = [i64, i64, i64] + [vp] * 14
        getattr(L, f"cmi_lobpcg_residual_{suf}").argtypes = [i64] + [vp] * 8     # cusp::eigen::lobpcg's vector tail (csrc/lobpcg.hip)
        getattr(L, f"cmi_lobpcg_gram_{suf}").argtypes = [i64] + [vp] * 9
        getattr(L, f"cmi_lobpcg_update_{suf}").argtypes = [i64, sc, sc, sc, c_int, sc] + [vp] * 11
        getattr(L, f"cmi_dense_gemm_{suf}").argtypes = [i64, i64, i64, vp, i64, vp, i64, vp, i64, vp]   # cusp::blas::gemm (csrc/dense.hip)
    L.cmi_count_zeros_f64.argtypes = [i64, vp, POINTER(c_int64), vp]
    L.cmi_count_zeros_f32.argtypes = [i64, vp, POINTER(c_int64), vp]
    L.cmi_tuning_hyb_rule.argtypes = [c_int, POINTER(c_int), POINTER(c_double), POINTER(c_int64)]
    L.cmi_tuning_set_hyb_rule.argtypes = [c_int, c_int, c_double, i64]
    L.cmi_tuning_waver_rule.argtypes = [c_int, POINTER(WaverRule)]
    L.cmi_tuning_set_waver_rule.argtypes = [c_int, POINTER(WaverRule)]
    L.cmi_tuning_hyb_light_speed.argtypes = [c_int, POINTER(c_double)]
    L.cmi_tuning_set_hyb_light_speed.argtypes = [c_int, c_double]
    L.cmi_hyb_entries_per_row.argtypes = [c_int, i64, vp, c_int, c_double, i64, POINTER(c_int64), vp]
    L.cmi_plan_create.argtypes = [c_int, c_int, i64, i64, i64, vp, cfgp, vp, POINTER(c_void_p)]
    L.cmi_plan_destroy.argtypes = [vp]
    L.cmi_plan_config.argtypes = [vp, cfgp]
    L.cmi_plan_validate.argtypes = [vp, vp, vp, vp, POINTER(c_int)]
    L.cmi_plan_info.argtypes = [vp, POINTER(c_int64), POINTER(c_int64), POINTER(c_int), POINTER(c_int)]
    L.cmi_plan_create_csr.argtypes = [c_int, i64, i64, i64, vp, vp, cfgp, vp, POINTER(c_void_p)]
    L.cmi_plan_create_coo.argtypes = [c_int, i64, i64, i64, vp, vp, cfgp, vp, POINTER(c_void_p)]
    L.cmi_plan_create_csr_values.argtypes = [c_int, i64, i64, i64, vp, vp, vp, cfgp, vp, POINTER(c_void_p)]
    L.cmi_plan_validate_values.argtypes = [vp, vp, vp, POINTER(c_int)]
    L.cmi_plan_device_bytes.argtypes = [vp, POINTER(c_int64)]
    L.cmi_plan_wavev_shift_tiles.argtypes = [vp, POINTER(c_int64)]
    L.cmi_set_index_compression.argtypes = [c_int]
    L.cmi_plan_hyb_launches.argtypes = [vp, POINTER(c_int)]
    L.cmi_plan_set_row_scale.argtypes = [vp, vp]
    L.cmi_plan_const_tiles.argtypes = [vp, POINTER(c_int64)]
    L.cmi_plan_drop_const_tiles.argtypes = [vp]
    L.cmi_plan_create_hyb.argtypes = [c_int, i64, i64, i64, i64, vp, cfgp, cfgp, vp, POINTER(c_void_p)]
    for suf in ("f64", "f32"):
        getattr(L, f"cmi_spmv_hyb_plan_{suf}").argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, vp]
        getattr(L, f"cmi_spmv_hyb_dot_plan_{suf}").argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    for suf in ("f64", "f32"):
        getattr(L, f"cmi_spmv_csr_plan_{suf}").argtypes = [vp, vp, vp, vp, vp, vp, i32, vp]
        getattr(L, f"cmi_spmv_coo_plan_{suf}").argtypes = [vp, vp, vp, vp, vp, vp, i32, vp]
        getattr(L, f"cmi_spmv_coo_dot_plan_{suf}").argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_spmv_csr_dot_plan_{suf}").argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.cmi_spmv_csr_dot_f32.argtypes = [i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, cfgp, vp]
    # communicator + collectives (RCCL behind the boundary)
    L.cmi_comm_unique_id.argtypes = [vp]
    L.cmi_comm_create.argtypes = [vp, c_int, c_int, POINTER(c_void_p)]
    L.cmi_comm_destroy.argtypes = [vp]
    L.cmi_comm_rank.argtypes = [vp, POINTER(c_int), POINTER(c_int)]
    L.cmi_comm_library_version.argtypes = [POINTER(c_int)]
    L.cmi_comm_barrier.argtypes = [vp, vp]
    L.cmi_comm_allgather_host.argtypes = [vp, vp, vp, c_size_t, vp]
    L.cmi_allreduce_f64.argtypes = [vp, vp, vp, i64, c_int, vp]
    for suf in ("f64", "f32"):
        getattr(L, f"cmi_allgather_{suf}").argtypes = [vp, vp, vp, i64, vp]
        getattr(L, f"cmi_allgatherv_{suf}").argtypes = [vp, vp, vp, POINTER(c_int64), POINTER(c_int64), c_int, vp]
        getattr(L, f"cmi_halo_exchange_{suf}").argtypes = [vp, vp, c_int, POINTER(c_int), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64),
                                                          POINTER(c_int64), vp]
    # the rest of BLAS-1 and the fused solver steps (csrc/blas1_extra.hip); scalars by value are c_double / c_float, the rest device pointers
    for suf, sc in (("f64", c_double), ("f32", c_float)):
        getattr(L, f"cmi_blas_scal_{suf}").argtypes = [i64, sc, vp, vp]
        getattr(L, f"cmi_blas_xmy_{suf}").argtypes = [i64, vp, vp, vp, vp]
        getattr(L, f"cmi_blas_axpbypcz_{suf}").argtypes = [i64, sc, vp, sc, vp, sc, vp, vp, vp]
        getattr(L, f"cmi_blas_asum_{suf}").argtypes = [i64, vp, vp, vp, vp]
        getattr(L, f"cmi_blas_amax_{suf}").argtypes = [i64, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_pcg_update_jacobi_{suf}").argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_pcg_direction_x_jacobi_{suf}").argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_bicgstab_s_{suf}").argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_bicgstab_xr_{suf}").argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_bicgstab_p_{suf}").argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_cr_xr_{suf}").argtypes = [i64, vp, vp, vp, vp, vp, vp, c_int, vp, vp, vp, vp]
        getattr(L, f"cmi_cr_py_{suf}").argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_blas_axpy_dot_{suf}").argtypes = [i64, vp, vp, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_blas_axpy_ratio_{suf}").argtypes = [i64, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_csr_diagonal_{suf}").argtypes = [i64, vp, vp, vp, vp, c_int, vp]
        # cusp::eigen's kernels (csrc/eigen.hip)
        getattr(L, f"cmi_csr_abs_row_sums_{suf}").argtypes = [i64, vp, vp, vp, c_int, vp]
        getattr(L, f"cmi_ell_abs_row_sums_{suf}").argtypes = [i64, i64, i64, i64, vp, vp, vp, vp, c_int, vp]
        getattr(L, f"cmi_dia_abs_row_sums_{suf}").argtypes = [i64, i64, i64, i64, vp, vp, vp, c_int, vp]
        getattr(L, f"cmi_random_fill_{suf}").argtypes = [i64, ctypes.c_uint64, vp, vp]
        getattr(L, f"cmi_blas_scal_recip_{suf}").argtypes = [i64, vp, c_int, vp, vp, vp]
    # host functions: the values cmi_random_fill_* writes
    L.cmi_random_hash.restype, L.cmi_random_hash.argtypes = ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]
    L.cmi_random_unit_f64.restype, L.cmi_random_unit_f64.argtypes = c_double, [ctypes.c_uint64]
    L.cmi_random_unit_f32.restype, L.cmi_random_unit_f32.argtypes = c_float, [ctypes.c_uint64]
    L.cmi_csr_column_span.argtypes = [i64, vp, POINTER(ctypes.c_int32), POINTER(ctypes.c_int32), vp]
    L.cmi_csr_rebase_offsets.argtypes = [i64, vp, ctypes.c_int32, vp, vp]
    # CSR x CSR (csrc/spgemm_csr.hip): the product comes back as a handle
    for suf in ("f64", "f32"):
        getattr(L, f"cmi_spgemm_csr_{suf}").argtypes = [i64, i64, i64, i64, vp, vp, vp, i64, vp, vp, vp, POINTER(c_void_p), vp]
        getattr(L, f"cmi_spgemm_take_{suf}").argtypes = [vp, vp, vp, vp, i64, vp]
    L.cmi_spgemm_num_entries.argtypes = [vp, POINTER(c_int64)]
    L.cmi_spgemm_info.argtypes = [vp, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]
    L.cmi_spgemm_destroy.argtypes = [vp]
    L.cmi_spgemm_limits.argtypes = [POINTER(c_int64), POINTER(c_int64)]
    L.cmi_spgemm_set_workspace.argtypes = [i64]
    # smoothed aggregation's set-up kernels (csrc/amg.hip)
    for suf, real in (("f64", c_double), ("f32", c_float)):
        getattr(L, f"cmi_csr_strength_symmetric_{suf}").argtypes = [i64, i64, i64, vp, vp, vp, c_double, vp, vp, vp, i64, vp]
        getattr(L, f"cmi_csr_scale_rows_{suf}").argtypes = [i64, i64, vp, vp, vp, real, vp, vp]
        getattr(L, f"cmi_aggregates_fit_{suf}").argtypes = [i64, i64, vp, vp, vp, vp, vp, i64, vp, vp]
        getattr(L, f"cmi_csr_elementwise_{suf}").argtypes = [i64, i64, i64, vp, vp, vp, i64, vp, vp, vp, c_int, vp, vp, vp, i64, POINTER(c_int), vp]
        getattr(L, f"cmi_relax_jacobi_presmooth_{suf}").argtypes = [i64, vp, vp, real, vp, vp]
    # evolution strength of connection (csrc/evolution.hip)
    L.cmi_csr_transpose_positions.argtypes = [i64, vp, vp, vp, POINTER(c_int), vp]
    for suf in ("f64", "f32"):
        getattr(L, f"cmi_csr_masked_product_{suf}").argtypes = [i64, vp, vp, vp, vp, vp, vp]
        getattr(L, f"cmi_csr_evolution_strength_{suf}").argtypes = [i64, i64, vp, vp, vp, vp, c_double, c_double, vp, vp, vp, i64, POINTER(c_int), vp]
    # the maximal independent set and its aggregation (csrc/mis.hip)
    L.cmi_csr_ring_max_u64.argtypes = [i64, i64, vp, vp, vp, vp, vp]
    # the semiring multiply (csrc/spmv_semiring.hip): ..., x, y0, init_value, combine, reduce, y, stream
    for suf, sc in (("f64", ctypes.c_double), ("f32", ctypes.c_float)):
        getattr(L, f"cmi_spmv_csr_semiring_{suf}").argtypes = [i64, i64, i64, vp, vp, vp, vp, vp, sc, i32, i32, vp, vp]
        getattr(L, f"cmi_spmv_coo_semiring_{suf}").argtypes = [i64, i64, i64, vp, vp, vp, vp, vp, sc, i32, i32, vp, vp]
        getattr(L, f"cmi_spmv_ell_semiring_{suf}").argtypes = [i64, i64, i64, i64, vp, vp, vp, vp, sc, i32, i32, vp, vp]
        getattr(L, f"cmi_spmv_dia_semiring_{suf}").argtypes = [i64, i64, i64, i64, vp, vp, vp, vp, sc, i32, i32, vp, vp]
    L.cmi_csr_maximal_independent_set.argtypes = [i64, i64, vp, vp, c_int, ctypes.c_uint64, vp, POINTER(c_int64), POINTER(c_int), vp]
    L.cmi_csr_mis_aggregate.argtypes = [i64, i64, vp, vp, ctypes.c_uint64, vp, vp, POINTER(c_int64), vp]
    # breadth-first search, pseudo-peripheral vertex, level ordering, gather / scatter (csrc/bfs.hip)
    L.cmi_bfs_levels_per_read.argtypes = []
    L.cmi_csr_breadth_first_search.argtypes = [i64, i64, vp, vp, i64, c_int, vp, POINTER(c_int64), POINTER(c_int), vp]
    L.cmi_csr_pseudo_peripheral_vertex.argtypes = [i64, i64, vp, vp, i64, vp, POINTER(c_int64), POINTER(c_int), vp]
    L.cmi_csr_symmetric_rcm.argtypes = [i64, i64, vp, vp, i64, vp, POINTER(c_int64), vp]
    for suf in ("i32", "f32", "f64"):
        getattr(L, f"cmi_gather_{suf}").argtypes = [i64, i64, vp, vp, vp, vp]
        getattr(L, f"cmi_scatter_{suf}").argtypes = [i64, i64, vp, vp, vp, vp]


def lib():
    """The loaded C-ABI library.  Raises (loudly) when it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError(
                f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C cusp-autotuned_amd/csrc`.  The SpMV engine has no CPU fallback.")
        # torch bundles its own HIP runtime (torch/lib/libamdhip64.so); it must be the one this
        # process binds, so import torch BEFORE the library pulls in /opt/rocm's copy.  Loading in the
        # other order leaves two runtimes fighting over the device ("no ROCm-capable device is
        # detected" at the first launch) -- seen on MI355X when a test module loaded the library first.
        import torch  # noqa: F401
        L = ctypes.CDLL(_LIB_PATH)
        _declare(L)
        _lib = L
    return _lib


def check(status):
    if status != 0:
        L = lib()
        raise CmiError(status, f"{L.cmi_status_string(status).decode()}: {L.cmi_last_error().decode()}")


def version():
    return lib().cmi_version()


# ------------------------------------------------------------------------------------------------
# tensor plumbing
# ------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else c_void_p(t.data_ptr())


def _suffix(t):
    import torch
    if t.dtype == torch.float64:
        return "f64"
    if t.dtype == torch.float32:
        return "f32"
    raise TypeError(f"value dtype must be float64 or float32, got {t.dtype}")


def _stream(stream):
    """hipStream_t of `stream` (a torch.cuda.Stream), default: torch's current stream."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    return c_void_p(stream.cuda_stream)


def _need(t, name, dtype=None):
    import torch
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA/HIP torch tensor (device memory); got {type(t).__name__}"
                        f"{'' if not isinstance(t, torch.Tensor) else ' on ' + str(t.device)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must have dtype {dtype}, got {t.dtype}")


def _cfg(cfg):
    return None if cfg is None else ctypes.byref(cfg)


def spmv_csr(num_rows, num_cols, Ap, Aj, Ax, x, y, accumulate=False, cfg=None, stream=None):
    import torch
    for t, n in ((Ap, "Ap"), (Aj, "Aj")):
        _need(t, n, torch.int32)
    for t, n in ((Ax, "Ax"), (x, "x"), (y, "y")):
        _need(t, n, y.dtype)
    if Ap.numel() != num_rows + 1 or x.numel() != num_cols or y.numel() != num_rows or Aj.numel() != Ax.numel():
        raise ValueError("spmv_csr: array lengths do not match the matrix shape")
    fn = getattr(lib(), "cmi_spmv_csr_" + _suffix(y))
    check(fn(num_rows, num_cols, Aj.numel(), _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(x), _ptr(y), int(bool(accumulate)),
             _cfg(cfg), _stream(stream)))


def spmm_csr(num_rows, num_cols, Ap, Aj, Ax, X, Y, accumulate=False, cfg=None, stream=None):
    """cmi_spmm_csr_*: Y = A X (or Y += A X) for 2-D tensors X (num_cols x k) and Y (num_rows x k).  Their stride() is
    passed as the C-ABI's element strides, so transposed views and column slices of wider tensors work as they are."""
    import torch
    for t, n in ((Ap, "Ap"), (Aj, "Aj")):
        _need(t, n, torch.int32)
    _need(Ax, "Ax", Y.dtype)
    for t, n in ((X, "X"), (Y, "Y")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise TypeError(f"{n} must be a CUDA/HIP torch tensor (device memory)")
        if t.dtype != Y.dtype:
            raise TypeError(f"{n} has dtype {t.dtype}, expected {Y.dtype}")
        if t.dim() != 2:
            raise ValueError(f"spmm_csr: {n} must be 2-D")
    if Ap.numel() != num_rows + 1 or Aj.numel() != Ax.numel() or X.shape[0] != num_cols or Y.shape[0] != num_rows or X.shape[1] != Y.shape[1]:
        raise ValueError("spmm_csr: array shapes do not match (X num_cols x k, Y num_rows x k)")
    fn = getattr(lib(), "cmi_spmm_csr_" + _suffix(Y))
    check(fn(num_rows, num_cols, Aj.numel(), _ptr(Ap), _ptr(Aj), _ptr(Ax), X.shape[1], _ptr(X), X.stride(0), X.stride(1),
             _ptr(Y), Y.stride(0), Y.stride(1), int(bool(accumulate)), _cfg(cfg), _stream(stream)))


def spgemm_limits():
    """cmi_spgemm_limits: (tile_products, workspace_products) in force now."""
    t, w = c_int64(0), c_int64(0)
    check(lib().cmi_spgemm_limits(byref(t), byref(w)))
    return int(t.value), int(w.value)


def spgemm_set_workspace(products):
    """cmi_spgemm_set_workspace: products per slab of every later cmi_spgemm_csr_* (process-wide); 0: the default."""
    check(lib().cmi_spgemm_set_workspace(int(products)))


def spgemm_csr(m, k, n, Ap, Aj, Ax, Bp, Bj, Bx, stream=None):
    """cmi_spgemm_csr_* + cmi_spgemm_take_*: C = A B for CSR arrays on the device.  Returns (Cp, Cj, Cx, info) with new
    tensors and info = what cmi_spgemm_info reported."""
    import torch
    for t, nm in ((Ap, "Ap"), (Aj, "Aj"), (Bp, "Bp"), (Bj, "Bj")):
        _need(t, nm, torch.int32)
    for t, nm in ((Ax, "Ax"), (Bx, "Bx")):
        _need(t, nm, Ax.dtype)
    if Ap.numel() != m + 1 or Bp.numel() != k + 1 or Aj.numel() != Ax.numel() or Bj.numel() != Bx.numel():
        raise ValueError("spgemm_csr: array lengths do not match the matrix shapes")
    suf = _suffix(Ax)
    L = lib()
    h = c_void_p()
    check(getattr(L, "cmi_spgemm_csr_" + suf)(m, k, n, Aj.numel(), _ptr(Ap), _ptr(Aj), _ptr(Ax), Bj.numel(), _ptr(Bp), _ptr(Bj), _ptr(Bx),
                                             byref(h), _stream(stream)))
    try:
        nnz, v = c_int64(0), [c_int64(0) for _ in range(4)]
        check(L.cmi_spgemm_num_entries(h, byref(nnz)))
        check(L.cmi_spgemm_info(h, *[byref(x) for x in v]))
        Cp = torch.empty(m + 1, dtype=torch.int32, device=Ax.device)
        Cj = torch.empty(nnz.value, dtype=torch.int32, device=Ax.device)
        Cx = torch.empty(nnz.value, dtype=Ax.dtype, device=Ax.device)
        check(getattr(L, "cmi_spgemm_take_" + suf)(h, _ptr(Cp), _ptr(Cj), _ptr(Cx), nnz.value, _stream(stream)))
        if stream is None:
            torch.cuda.current_stream().synchronize()  # the handle's pieces are read by the copies: finish before it goes
        else:
            stream.synchronize()
    finally:
        check(L.cmi_spgemm_destroy(h))
    info = dict(zip(("products", "slabs", "rows_in_tiles", "rows_in_slabs"), (int(x.value) for x in v)))
    return Cp, Cj, Cx, info


# ------------------------------------------------------------------------------------------------
# smoothed aggregation's set-up kernels (csrc/amg.hip).  Outputs are new tensors cut to the entry count.
# ------------------------------------------------------------------------------------------------
def csr_strength_symmetric(num_rows, Ap, Aj, Ax, theta=0.0, stream=None):
    """cmi_csr_strength_symmetric_*: the entries of the square CSR matrix A with |A_ij| >= theta * sqrt(|A_ii| |A_jj|), in
    storage order.  Returns (Sp, Sj, Sx)."""
    import torch
    for t, nm in ((Ap, "Ap"), (Aj, "Aj")):
        _need(t, nm, torch.int32)
    _need(Ax, "Ax")
    if Ap.numel() != num_rows + 1 or Aj.numel() != Ax.numel():
        raise ValueError("csr_strength_symmetric: array lengths do not match the matrix shape")
    nnz = Aj.numel()
    Sp = torch.empty(num_rows + 1, dtype=torch.int32, device=Ax.device)
    Sj = torch.empty(nnz, dtype=torch.int32, device=Ax.device)
    Sx = torch.empty(nnz, dtype=Ax.dtype, device=Ax.device)
    check(getattr(lib(), "cmi_csr_strength_symmetric_" + _suffix(Ax))(num_rows, num_rows, nnz, _ptr(Ap), _ptr(Aj), _ptr(Ax), float(theta), _ptr(Sp),
                                                                      _ptr(Sj), _ptr(Sx), nnz, _stream(stream)))
    kept = int(Sp[num_rows].item())
    return Sp, Sj[:kept].clone(), Sx[:kept].clone()


def csr_transpose_positions(num_rows, Ap, Aj, stream=None):
    """cmi_csr_transpose_positions: tpos[e] = the position of the entry (col(e), row(e)) of a square CSR pattern.  Returns tpos,
    or None when the pattern does not conform (not symmetric, a row not strictly ascending, a column outside the matrix)."""
    import torch
    for t, nm in ((Ap, "Ap"), (Aj, "Aj")):
        _need(t, nm, torch.int32)
    if Ap.numel() != num_rows + 1:
        raise ValueError("csr_transpose_positions: array lengths do not match the matrix shape")
    tpos = torch.empty(Aj.numel(), dtype=torch.int32, device=Aj.device)
    ok = c_int(0)
    check(lib().cmi_csr_transpose_positions(num_rows, _ptr(Ap), _ptr(Aj), _ptr(tpos), byref(ok), _stream(stream)))
    return tpos if ok.value else None


def csr_masked_product(num_rows, Ap, Aj, Vx, Wx, out=None, stream=None):
    """cmi_csr_masked_product_*: out[e] = the sum of Vx[p] * Wx[q] over the columns that rows row(e) and col(e) have in common,
    in ascending column order from +0.  Returns out (a new tensor unless given)."""
    import torch
    for t, nm in ((Ap, "Ap"), (Aj, "Aj")):
        _need(t, nm, torch.int32)
    if out is None:
        out = torch.empty_like(Vx)
    for t, nm in ((Vx, "Vx"), (Wx, "Wx"), (out, "out")):
        _need(t, nm, Vx.dtype)
    if Ap.numel() != num_rows + 1 or not (Aj.numel() == Vx.numel() == Wx.numel() == out.numel()):
        raise ValueError("csr_masked_product: array lengths do not match the matrix shape")
    check(getattr(lib(), "cmi_csr_masked_product_" + _suffix(Vx))(num_rows, _ptr(Ap), _ptr(Aj), _ptr(Vx), _ptr(Wx), _ptr(out), _stream(stream)))
    return out


def csr_evolution_strength(num_rows, Ap, Aj, Ax, B_, rho_DinvA, epsilon=4.0, stream=None):
    """cmi_csr_evolution_strength_*: the evolution measure of the square CSR matrix A for the candidate vector B and a given
    non-zero rho(D^-1 A).  Returns (Sp, Sj, Sx), the kept entries in storage order with their final values, or None when the
    pattern does not conform (see csr_transpose_positions)."""
    import torch
    for t, nm in ((Ap, "Ap"), (Aj, "Aj")):
        _need(t, nm, torch.int32)
    _need(Ax, "Ax")
    _need(B_, "B", Ax.dtype)
    if Ap.numel() != num_rows + 1 or Aj.numel() != Ax.numel() or B_.numel() != num_rows:
        raise ValueError("csr_evolution_strength: array lengths do not match the matrix shape")
    nnz = Aj.numel()
    Sp = torch.empty(num_rows + 1, dtype=torch.int32, device=Ax.device)
    Sj = torch.empty(nnz, dtype=torch.int32, device=Ax.device)
    Sx = torch.empty(nnz, dtype=Ax.dtype, device=Ax.device)
    ok = c_int(0)
    check(getattr(lib(), "cmi_csr_evolution_strength_" + _suffix(Ax))(num_rows, nnz, _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(B_), float(rho_DinvA), float(epsilon),
                                                                      _ptr(Sp), _ptr(Sj), _ptr(Sx), nnz, byref(ok), _stream(stream)))
    if not ok.value:
        return None
    kept = int(Sp[num_rows].item())
    return Sp, Sj[:kept].clone(), Sx[:kept].clone()


def csr_scale_rows(num_rows, Ap, Ax, d, lam, out=None, stream=None):
    """cmi_csr_scale_rows_*: out[e] = (Ax[e] / d[row(e)]) * lam; out=None: a new tensor, out=Ax: in place."""
    import torch
    _need(Ap, "Ap", torch.int32)
    if out is None:
        out = torch.empty_like(Ax)
    for t, nm in ((Ax, "Ax"), (d, "d"), (out, "out")):
        _need(t, nm, Ax.dtype)
    if Ap.numel() != num_rows + 1 or d.numel() != num_rows or out.numel() != Ax.numel():
        raise ValueError("csr_scale_rows: array lengths do not match the matrix shape")
    check(getattr(lib(), "cmi_csr_scale_rows_" + _suffix(Ax))(num_rows, Ax.numel(), _ptr(Ap), _ptr(Ax), _ptr(d), float(lam), _ptr(out), _stream(stream)))
    return out


def aggregates_fit(aggregates, B_, num_aggregates, stream=None):
    """cmi_aggregates_fit_*: the tentative prolongator of one candidate vector.  Returns (Tp, Tj, Tx, R); aggregates[i] == -1
    leaves row i empty, an id outside [-1, num_aggregates) raises CmiError."""
    import torch
    _need(aggregates, "aggregates", torch.int32)
    _need(B_, "B")
    n = aggregates.numel()
    if B_.numel() != n:
        raise ValueError("aggregates_fit: aggregates and B must have the same length")
    Tp = torch.empty(n + 1, dtype=torch.int32, device=B_.device)
    Tj = torch.empty(n, dtype=torch.int32, device=B_.device)
    Tx = torch.empty(n, dtype=B_.dtype, device=B_.device)
    R = torch.empty(num_aggregates, dtype=B_.dtype, device=B_.device)
    check(getattr(lib(), "cmi_aggregates_fit_" + _suffix(B_))(n, num_aggregates, _ptr(aggregates), _ptr(B_), _ptr(Tp), _ptr(Tj), _ptr(Tx), n, _ptr(R),
                                                              _stream(stream)))
    kept = int(Tp[n].item())
    return Tp, Tj[:kept].clone(), Tx[:kept].clone(), R


def csr_elementwise(num_rows, num_cols, Ap, Aj, Ax, Bp, Bj, Bx, op="add", stream=None):
    """cmi_csr_elementwise_*: C = A + B (op "add") or A - B ("subtract") for CSR operands with rows sorted by column.  Returns
    (Cp, Cj, Cx), or None when an operand is not sorted (nothing was computed: sort it first)."""
    import torch
    for t, nm in ((Ap, "Ap"), (Aj, "Aj"), (Bp, "Bp"), (Bj, "Bj")):
        _need(t, nm, torch.int32)
    for t, nm in ((Ax, "Ax"), (Bx, "Bx")):
        _need(t, nm, Ax.dtype)
    if op not in ("add", "subtract"):
        raise ValueError("csr_elementwise: op is 'add' or 'subtract'")
    if Ap.numel() != num_rows + 1 or Bp.numel() != num_rows + 1 or Aj.numel() != Ax.numel() or Bj.numel() != Bx.numel():
        raise ValueError("csr_elementwise: array lengths do not match the matrix shape")
    cap = Aj.numel() + Bj.numel()
    Cp = torch.empty(num_rows + 1, dtype=torch.int32, device=Ax.device)
    Cj = torch.empty(cap, dtype=torch.int32, device=Ax.device)
    Cx = torch.empty(cap, dtype=Ax.dtype, device=Ax.device)
    ok = c_int(0)
    check(getattr(lib(), "cmi_csr_elementwise_" + _suffix(Ax))(num_rows, num_cols, Aj.numel(), _ptr(Ap), _ptr(Aj), _ptr(Ax), Bj.numel(), _ptr(Bp), _ptr(Bj),
                                                               _ptr(Bx), int(op == "subtract"), _ptr(Cp), _ptr(Cj), _ptr(Cx), cap, byref(ok), _stream(stream)))
    if not ok.value:
        return None
    kept = int(Cp[num_rows].item())
    return Cp, Cj[:kept].clone(), Cx[:kept].clone()


def relax_jacobi_presmooth(diag, b, omega, x, stream=None):
    """cmi_relax_jacobi_presmooth_*: x[i] = (omega * b[i]) / diag[i] -- a Jacobi sweep from x = 0."""
    for t, n in ((diag, "diag"), (b, "b"), (x, "x")):
        _need(t, n, x.dtype)
    if diag.numel() != x.numel() or b.numel() != x.numel():
        raise ValueError("relax_jacobi_presmooth: vectors must have the same length")
    check(getattr(lib(), "cmi_relax_jacobi_presmooth_" + _suffix(x))(x.numel(), _ptr(diag), _ptr(b), float(omega), _ptr(x), _stream(stream)))


def _pattern(A, who):
    """(num_rows, Ap, Aj) of a square CSR pattern given as (num_rows, Ap, Aj) or as an object with row_offsets / column_indices."""
    import torch
    if isinstance(A, (tuple, list)):
        num_rows, Ap, Aj = A
    else:
        if getattr(A, "num_rows", None) != getattr(A, "num_cols", None):
            raise ValueError(f"{who}: matrix must be square")
        num_rows, Ap, Aj = A.num_rows, A.row_offsets, A.column_indices
    for t, nm in ((Ap, "Ap"), (Aj, "Aj")):
        _need(t, nm, torch.int32)
    if Ap.numel() != num_rows + 1:
        raise ValueError(f"{who}: array lengths do not match the matrix shape")
    return int(num_rows), Ap, Aj


def csr_ring_max(num_rows, Ap, Aj, x, z=None, stream=None):
    """cmi_csr_ring_max_u64: z[i] = max(x[i], max over row i of x[Aj[jj]]) on 64-bit keys (int64 tensors holding the
    unsigned bits).  z=None: a new tensor; z must not be x."""
    import torch
    num_rows, Ap, Aj = _pattern((num_rows, Ap, Aj), "csr_ring_max")
    if z is None:
        z = torch.empty_like(x)
    for t, nm in ((x, "x"), (z, "z")):
        _need(t, nm, torch.int64)
    if x.numel() != num_rows or z.numel() != num_rows:
        raise ValueError("csr_ring_max: x and z must have num_rows elements")
    check(lib().cmi_csr_ring_max_u64(num_rows, Aj.numel(), _ptr(Ap), _ptr(Aj), _ptr(x), _ptr(z), _stream(stream)))
    return z


def maximal_independent_set(A, k=1, seed=0, stream=None):
    """cmi_csr_maximal_independent_set: MIS(k) of the graph whose edges are the stored entries of the square CSR matrix A
    (a CSR matrix object, or (num_rows, Ap, Aj)).  Returns (stencil int32 0/1, set_size, rounds)."""
    import torch
    num_rows, Ap, Aj = _pattern(A, "maximal_independent_set")
    stencil = torch.empty(num_rows, dtype=torch.int32, device=Ap.device)
    size, rounds = c_int64(0), c_int(0)
    check(lib().cmi_csr_maximal_independent_set(num_rows, Aj.numel(), _ptr(Ap), _ptr(Aj), int(k), int(seed), _ptr(stencil), byref(size), byref(rounds),
                                                _stream(stream)))
    return stencil, int(size.value), int(rounds.value)


def mis_aggregate(C, seed=0, stream=None):
    """cmi_csr_mis_aggregate: aggregates of the strength matrix C (a CSR matrix object, or (num_rows, Ap, Aj)) from MIS(2).
    Returns (aggregates int32 with -1 for a node in no aggregate, mis int32 0/1, num_aggregates)."""
    import torch
    num_rows, Ap, Aj = _pattern(C, "mis_aggregate")
    aggregates = torch.empty(num_rows, dtype=torch.int32, device=Ap.device)
    mis = torch.empty(num_rows, dtype=torch.int32, device=Ap.device)
    count = c_int64(0)
    check(lib().cmi_csr_mis_aggregate(num_rows, Aj.numel(), _ptr(Ap), _ptr(Aj), int(seed), _ptr(aggregates), _ptr(mis), byref(count), _stream(stream)))
    return aggregates, mis, int(count.value)


def bfs_levels_per_read():
    """cmi_bfs_levels_per_read: the expansion launches of a search between two host reads of its counters."""
    return int(lib().cmi_bfs_levels_per_read())


def breadth_first_search(n, Ap, Aj, src, mark_levels=True, stream=None):
    """cmi_csr_breadth_first_search from `src` on the stored pattern (n, Ap, Aj) of a square CSR matrix, edges directed along
    the rows.  Returns (labels int32, reached, depth): the levels (-1: not reached), or with mark_levels=False the
    predecessors (-2 the source, -1 not reached, else the smallest-numbered vertex of the previous level with an edge to it)."""
    import torch
    n, Ap, Aj = _pattern((n, Ap, Aj), "breadth_first_search")
    labels = torch.empty(n, dtype=torch.int32, device=Ap.device)
    reached, depth = c_int64(0), c_int(0)
    check(lib().cmi_csr_breadth_first_search(n, Aj.numel(), _ptr(Ap), _ptr(Aj), int(src), int(bool(mark_levels)), _ptr(labels), byref(reached), byref(depth),
                                             _stream(stream)))
    return labels, int(reached.value), int(depth.value)


def pseudo_peripheral_vertex(n, Ap, Aj, start=0, stream=None):
    """cmi_csr_pseudo_peripheral_vertex: searches from `start` until the depth stops growing.  Returns (vertex, levels int32
    of the last search, searches)."""
    import torch
    n, Ap, Aj = _pattern((n, Ap, Aj), "pseudo_peripheral_vertex")
    levels = torch.empty(n, dtype=torch.int32, device=Ap.device)
    vertex, searches = c_int64(0), c_int(0)
    check(lib().cmi_csr_pseudo_peripheral_vertex(n, Aj.numel(), _ptr(Ap), _ptr(Aj), int(start), _ptr(levels), byref(vertex), byref(searches), _stream(stream)))
    return int(vertex.value), levels, int(searches.value)


def symmetric_rcm(n, Ap, Aj, start=0, stream=None):
    """cmi_csr_symmetric_rcm: the level ordering from a pseudo-peripheral vertex.  Returns (permutation int32 with
    permutation[v] = the new number of v, vertex)."""
    import torch
    n, Ap, Aj = _pattern((n, Ap, Aj), "symmetric_rcm")
    permutation = torch.empty(n, dtype=torch.int32, device=Ap.device)
    vertex = c_int64(0)
    check(lib().cmi_csr_symmetric_rcm(n, Aj.numel(), _ptr(Ap), _ptr(Aj), int(start), _ptr(permutation), byref(vertex), _stream(stream)))
    return permutation, int(vertex.value)


def _map_copy(kind, map, x, m, stream):
    import torch
    _need(map, "map", torch.int32)
    _need(x, "x")
    suffix = "i32" if x.dtype == torch.int32 else _suffix(x)
    n = map.numel()
    if x.numel() != (m if kind == "gather" else n):
        raise ValueError(f"{kind}: x must have {'m' if kind == 'gather' else 'as many'} elements{'' if kind == 'gather' else ' as map'}")
    out = torch.empty(n if kind == "gather" else m, dtype=x.dtype, device=x.device)
    check(getattr(lib(), f"cmi_{kind}_{suffix}")(n, int(m), _ptr(map), _ptr(x), _ptr(out), _stream(stream)))
    return out


def gather(map, x, m, stream=None):
    """cmi_gather_*: out[i] = x[map[i]]; x has m elements (int32, float32 or float64), map is int32 with entries in [0, m)."""
    return _map_copy("gather", map, x, m, stream)


def scatter(map, x, m, stream=None):
    """cmi_scatter_*: out[map[i]] = x[i]; out has m elements (those no entry names are left uninitialised), map is int32 with
    entries in [0, m)."""
    return _map_copy("scatter", map, x, m, stream)


def _plan_handle(plan):
    return None if plan is None else plan.handle


def spmv_csr_axpby(num_rows, num_cols, Ap, Aj, Ax, x, alpha, beta, z, out, plan=None, stream=None):
    """cmi_spmv_csr_axpby_*: out[i] = alpha * (A x)[i] + beta * z[i] in one launch (out may be z, never x).  alpha = -1,
    beta = 1, z = b: the residual; alpha = 1, beta = c, z = residual: the polynomial smoother's step."""
    import torch
    for t, n in ((Ap, "Ap"), (Aj, "Aj")):
        _need(t, n, torch.int32)
    for t, n in ((Ax, "Ax"), (x, "x"), (z, "z"), (out, "out")):
        _need(t, n, out.dtype)
    if Ap.numel() != num_rows + 1 or x.numel() != num_cols or z.numel() != num_rows or out.numel() != num_rows or Aj.numel() != Ax.numel():
        raise ValueError("spmv_csr_axpby: array lengths do not match the matrix shape")
    fn = getattr(lib(), "cmi_spmv_csr_axpby_" + _suffix(out))
    check(fn(_plan_handle(plan), num_rows, num_cols, Aj.numel(), _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(x), alpha, beta, _ptr(z), _ptr(out),
             _stream(stream)))


def csr_jacobi_sweep(num_rows, Ap, Aj, Ax, diag, b, x, omega, x_out, plan=None, stream=None):
    """cmi_csr_jacobi_sweep_*: x_out[i] = x[i] + omega * (b[i] - (A x)[i]) / diag[i] in one launch (square A; x_out is not x)."""
    import torch
    for t, n in ((Ap, "Ap"), (Aj, "Aj")):
        _need(t, n, torch.int32)
    for t, n in ((Ax, "Ax"), (diag, "diag"), (b, "b"), (x, "x"), (x_out, "x_out")):
        _need(t, n, x_out.dtype)
    if Ap.numel() != num_rows + 1 or Aj.numel() != Ax.numel() or any(t.numel() != num_rows for t in (diag, b, x, x_out)):
        raise ValueError("csr_jacobi_sweep: array lengths do not match the matrix shape")
    fn = getattr(lib(), "cmi_csr_jacobi_sweep_" + _suffix(x_out))
    check(fn(_plan_handle(plan), num_rows, Aj.numel(), _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(diag), _ptr(b), _ptr(x), omega, _ptr(x_out),
             _stream(stream)))


def relax_jacobi_update(diag, b, y, omega, x, stream=None):
    """cmi_relax_jacobi_update_*: x[i] = x[i] + omega * (b[i] - y[i]) / diag[i], in place (y = A x from any format's multiply)."""
    for t, n in ((diag, "diag"), (b, "b"), (y, "y"), (x, "x")):
        _need(t, n, x.dtype)
    if any(t.numel() != x.numel() for t in (diag, b, y)):
        raise ValueError("relax_jacobi_update: vectors must have the same length")
    fn = getattr(lib(), "cmi_relax_jacobi_update_" + _suffix(x))
    check(fn(x.numel(), _ptr(diag), _ptr(b), _ptr(y), omega, _ptr(x), _stream(stream)))


def csr_gauss_seidel_colour(num_rows, Ap, Aj, Ax, b, x, ordering, slot_begin, slot_end, scratch=None, stream=None):
    """cmi_csr_gauss_seidel_colour_*: one colour of a Gauss-Seidel sweep, in place.  For every slot s of [slot_begin, slot_end),
    i = ordering[s]: x[i] = (b[i] - sum of row i without its diagonal entry) / A(i, i), left as it is where the row stores no
    non-zero diagonal.  scratch=None: one launch, and no row of the range may hold an off-diagonal column of the range;
    scratch (at least slot_end - slot_begin values): two launches, every row reads the x from before the call."""
    import torch
    for t, n in ((Ap, "Ap"), (Aj, "Aj"), (ordering, "ordering")):
        _need(t, n, torch.int32)
    for t, n in ((Ax, "Ax"), (b, "b"), (x, "x"), (scratch, "scratch")):
        _need(t, n, x.dtype)
    if Ap.numel() != num_rows + 1 or Aj.numel() != Ax.numel() or b.numel() != num_rows or x.numel() != num_rows:
        raise ValueError("csr_gauss_seidel_colour: array lengths do not match the matrix shape")
    if slot_end > ordering.numel() or (scratch is not None and scratch.numel() < slot_end - slot_begin):
        raise ValueError("csr_gauss_seidel_colour: ordering or scratch is shorter than the slot range")
    fn = getattr(lib(), "cmi_csr_gauss_seidel_colour_" + _suffix(x))
    check(fn(num_rows, Aj.numel(), _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(b), _ptr(x), _ptr(ordering), int(slot_begin), int(slot_end),
             _ptr(scratch), _stream(stream)))


class Plan:
    """cmi_plan: what the library learns about one matrix before its first multiply (launch shape; CSR: row-length
    profile; COO: row-sortedness).  Creating one synchronises the stream; multiplies through it never do."""

    def __init__(self, fmt, dtype, num_rows, num_cols, num_entries, index_array=None, cfg=None, stream=None):
        import torch
        self._h = c_void_p()
        if index_array is not None:
            _need(index_array, "index_array", torch.int32)
        code = F64 if dtype in (F64, torch.float64) else F32
        check(lib().cmi_plan_create(fmt, code, num_rows, num_cols, num_entries, _ptr(index_array), _cfg(cfg), _stream(stream),
                                    byref(self._h)))
        self.format, self.dtype = fmt, code
        self.num_rows, self.num_cols, self.num_entries = num_rows, num_cols, num_entries

    @classmethod
    def csr(cls, dtype, num_rows, num_cols, Ap, Aj, cfg=None, stream=None):
        """cmi_plan_create_csr: a CSR plan made from both structure arrays -- with cfg.kernel == CSR_STREAM_C16 (or after
        set_index_compression(True)) it also builds the 16-bit column copy; config().kernel tells whether it was granted."""
        import torch
        self = cls.__new__(cls)
        self._h = c_void_p()
        _need(Ap, "Ap", torch.int32)
        _need(Aj, "Aj", torch.int32)
        if Ap.numel() != num_rows + 1:
            raise ValueError("Plan.csr: row offsets must have num_rows + 1 entries")
        code = F64 if dtype in (F64, torch.float64) else F32
        check(lib().cmi_plan_create_csr(code, num_rows, num_cols, Aj.numel(), _ptr(Ap), _ptr(Aj), _cfg(cfg), _stream(stream), byref(self._h)))
        self.format, self.dtype = FORMAT_CSR, code
        self.num_rows, self.num_cols, self.num_entries = num_rows, num_cols, Aj.numel()
        return self

    @classmethod
    def coo(cls, dtype, num_rows, num_cols, Ai, Aj, cfg=None, stream=None):
        """cmi_plan_create_coo: a COO plan made from both index arrays -- sorted entries get a CSR sub-plan made with the columns (the
        run-compressed copy where the columns come in runs)."""
        import torch
        self = cls.__new__(cls)
        self._h = c_void_p()
        _need(Ai, "Ai", torch.int32)
        _need(Aj, "Aj", torch.int32)
        if Ai.numel() != Aj.numel():
            raise ValueError("Plan.coo: row and column indices must have the same length")
        code = F64 if dtype in (F64, torch.float64) else F32
        check(lib().cmi_plan_create_coo(code, num_rows, num_cols, Aj.numel(), _ptr(Ai), _ptr(Aj), _cfg(cfg), _stream(stream), byref(self._h)))
        self.format, self.dtype = FORMAT_COO, code
        self.num_rows, self.num_cols, self.num_entries = num_rows, num_cols, Aj.numel()
        return self

    @classmethod
    def csr_values(cls, num_rows, num_cols, Ap, Aj, Ax, cfg=None, stream=None):
        """cmi_plan_create_csr_values: Plan.csr plus the values -- with cfg.kernel == CSR_STREAM_PACKED the plan copies pieces AND values into
        one span per wave tile (the plan then owns a copy of the values: validate_values tells whether they have changed since).  With cfg None
        (or an AUTO kernel) a plan that keeps csr_wavev's shift table also marks its CONSTANT tiles (const_tiles()): marks only, the values are
        read live; after a non-uniform in-place edit of the values ask validate_values and drop_const_tiles() if it says False."""
        import torch
        self = cls.__new__(cls)
        self._h = c_void_p()
        _need(Ap, "Ap", torch.int32)
        _need(Aj, "Aj", torch.int32)
        if Ap.numel() != num_rows + 1 or Ax.numel() != Aj.numel():
            raise ValueError("Plan.csr_values: row offsets must have num_rows + 1 entries, values as many as columns")
        code = F64 if Ax.dtype == torch.float64 else F32
        check(lib().cmi_plan_create_csr_values(code, num_rows, num_cols, Aj.numel(), _ptr(Ap), _ptr(Aj), _ptr(Ax), _cfg(cfg), _stream(stream), byref(self._h)))
        self.format, self.dtype = FORMAT_CSR, code
        self.num_rows, self.num_cols, self.num_entries = num_rows, num_cols, Aj.numel()
        return self

    def validate_values(self, values, stream=None):
        """cmi_plan_validate_values: False when a CSR_STREAM_PACKED plan's copy of the values no longer matches `values`, or when a tile the
        plan marked constant no longer has identical rows in `values`."""
        ok = c_int(-1)
        check(lib().cmi_plan_validate_values(self._h, _ptr(values), _stream(stream), byref(ok)))
        return bool(ok.value)

    def device_bytes(self):
        n = c_int64()
        check(lib().cmi_plan_device_bytes(self._h, byref(n)))
        return n.value

    def shifted_tiles(self):
        """cmi_plan_wavev_shift_tiles: the wave tiles a csr_wavev plan with the 16-bit column copy multiplies without reading a column
        (rows of the tile = its first row's columns moved along with the row); 0 when the plan keeps no such table."""
        n = c_int64()
        check(lib().cmi_plan_wavev_shift_tiles(self._h, byref(n)))
        return n.value

    def const_tiles(self):
        """cmi_plan_const_tiles: the wave tiles multiplied from their first row's values alone; 0 when the plan keeps no marks."""
        n = c_int64()
        check(lib().cmi_plan_const_tiles(self._h, byref(n)))
        return n.value

    def drop_const_tiles(self):
        """cmi_plan_drop_const_tiles: frees the marks; the plan then multiplies as one made without the values."""
        check(lib().cmi_plan_drop_const_tiles(self._h))

    @classmethod
    def hyb(cls, dtype, num_rows, num_cols, width, coo_row_indices, cfg_ell=None, cfg_coo=None, stream=None):
        """cmi_plan_create_hyb: both parts' launch shapes and -- COO part sorted by row -- the per-tile entry ranges of the
        one-launch HYB kernel (spmv_hyb_plan)."""
        import torch
        self = cls.__new__(cls)
        self._h = c_void_p()
        _need(coo_row_indices, "coo_row_indices", torch.int32)
        code = F64 if dtype in (F64, torch.float64) else F32
        check(lib().cmi_plan_create_hyb(code, num_rows, num_cols, width, coo_row_indices.numel(), _ptr(coo_row_indices),
                                        _cfg(cfg_ell), _cfg(cfg_coo), _stream(stream), byref(self._h)))
        self.format, self.dtype = FORMAT_HYB, code
        self.num_rows, self.num_cols, self.num_entries = num_rows, num_cols, num_rows * width
        self.width, self.coo_entries = width, coo_row_indices.numel()
        return self

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.cmi_plan_destroy(h)

    @property
    def handle(self):
        return self._h

    def validate(self, index_array, column_indices=None, stream=None):
        """cmi_plan_validate: True while the arrays the plan was made from still hold what they held then (one streaming pass
        over them + a stream synchronisation); False after an in-place edit -- make a new plan."""
        ok = c_int(-1)
        check(lib().cmi_plan_validate(self._h, _ptr(index_array), _ptr(column_indices), _stream(stream), byref(ok)))
        return bool(ok.value)

    def hyb_launches(self):
        """1 = the one-launch HYB kernel (or an empty COO part), 2 = ELL kernel + COO kernel."""
        n = c_int()
        check(lib().cmi_plan_hyb_launches(self._h, byref(n)))
        return n.value

    def config(self):
        c = Config()
        check(lib().cmi_plan_config(self._h, byref(c)))
        return c

    def info(self):
        """dict: max_row_length, entries_in_long_rows (CSR; -1 otherwise), coo_sorted (COO: True/False, else None),
        storage_order_sums (every result bit-identical to the host loop?) and -- only while the plan keeps constant-tile marks --
        constant_tiles (const_tiles(); a plan without marks has no such key: info().get("constant_tiles", 0))."""
        a, b, s, e = c_int64(), c_int64(), c_int(), c_int()
        check(lib().cmi_plan_info(self._h, byref(a), byref(b), byref(s), byref(e)))
        out = {"max_row_length": a.value, "entries_in_long_rows": b.value,
               "coo_sorted": None if s.value < 0 else bool(s.value), "storage_order_sums": bool(e.value)}
        const = self.const_tiles()
        if const:
            out["constant_tiles"] = const
        return out


def spmv_csr_plan(plan, Ap, Aj, Ax, x, y, accumulate=False, stream=None):
    """cmi_spmv_csr_plan_*: the multiply steered by a plan (no table lookup, no measurement, no sync)."""
    import torch
    for t, n in ((Ap, "Ap"), (Aj, "Aj")):
        _need(t, n, torch.int32)
    for t, n in ((Ax, "Ax"), (x, "x"), (y, "y")):
        _need(t, n, y.dtype)
    if (Ap.numel() != plan.num_rows + 1 or x.numel() != plan.num_cols or y.numel() != plan.num_rows
            or Aj.numel() != plan.num_entries or Ax.numel() != plan.num_entries):
        raise ValueError("spmv_csr_plan: array lengths do not match the plan's matrix shape")
    fn = getattr(lib(), "cmi_spmv_csr_plan_" + _suffix(y))
    check(fn(plan.handle, _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(x), _ptr(y), int(bool(accumulate)), _stream(stream)))


def spmv_coo_plan(plan, Ai, Aj, Ax, x, y, accumulate=False, stream=None):
    import torch
    for t, n in ((Ai, "Ai"), (Aj, "Aj")):
        _need(t, n, torch.int32)
    for t, n in ((Ax, "Ax"), (x, "x"), (y, "y")):
        _need(t, n, y.dtype)
    if (Ai.numel() != plan.num_entries or Aj.numel() != plan.num_entries or Ax.numel() != plan.num_entries
            or x.numel() != plan.num_cols or y.numel() != plan.num_rows):
        raise ValueError("spmv_coo_plan: array lengths do not match the plan's matrix shape")
    fn = getattr(lib(), "cmi_spmv_coo_plan_" + _suffix(y))
    check(fn(plan.handle, _ptr(Ai), _ptr(Aj), _ptr(Ax), _ptr(x), _ptr(y), int(bool(accumulate)), _stream(stream)))


def spmv_csr_dot(num_rows, num_cols, Ap, Aj, Ax, x, y, w, result, workspace, cfg=None, stream=None, plan=None):
    """y <- A x and result[0] <- <y, w> in one pass (cmi_spmv_csr_dot_{f64,f32}[_plan]); result is a float64 tensor
    for both value types (f32: products and partial sums accumulate in double)."""
    import torch
    for t, n in ((Ap, "Ap"), (Aj, "Aj")):
        _need(t, n, torch.int32)
    for t, n in ((Ax, "Ax"), (x, "x"), (y, "y"), (w, "w")):
        _need(t, n, y.dtype)
    _need(result, "result", torch.float64)
    if (Ap.numel() != num_rows + 1 or x.numel() != num_cols or y.numel() != num_rows or w.numel() != num_rows
            or Aj.numel() != Ax.numel() or result.numel() < 1):
        raise ValueError("spmv_csr_dot: array lengths do not match the matrix shape")
    suf = _suffix(y)
    if plan is not None:
        check(getattr(lib(), "cmi_spmv_csr_dot_plan_" + suf)(plan.handle, _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(x), _ptr(y), _ptr(w),
                                                             _ptr(result), _ptr(workspace), _stream(stream)))
    else:
        check(getattr(lib(), "cmi_spmv_csr_dot_" + suf)(num_rows, num_cols, Aj.numel(), _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(x), _ptr(y),
                                                        _ptr(w), _ptr(result), _ptr(workspace), _cfg(cfg), _stream(stream)))


def spmv_ell_dot(num_rows, num_cols, width, pitch, Aj, Ax, x, y, w, result, workspace, row_lengths=None, cfg=None, stream=None):
    """ELL: y <- A x and result[0] <- <y, w> (a double) in one pass (cmi_spmv_ell_dot_{f64,f32})."""
    import torch
    for t, n in ((Ax, "Ax"), (x, "x"), (y, "y"), (w, "w")):
        _need(t, n, y.dtype)
    _need(result, "result", torch.float64)
    _need(Aj, "Aj", torch.int32)
    if x.numel() != num_cols or y.numel() != num_rows or w.numel() != num_rows or Aj.numel() < width * pitch or Ax.numel() < width * pitch:
        raise ValueError("spmv_ell_dot: array lengths do not match the matrix shape")
    check(getattr(lib(), "cmi_spmv_ell_dot_" + _suffix(y))(num_rows, num_cols, width, pitch, _ptr(Aj), _ptr(Ax), _ptr(row_lengths), _ptr(x), _ptr(y),
                                                           _ptr(w), _ptr(result), _ptr(workspace), _cfg(cfg), _stream(stream)))


def spmv_dia_dot(num_rows, num_cols, num_diagonals, pitch, offsets, values, x, y, w, result, workspace, cfg=None, stream=None):
    """DIA: y <- A x and result[0] <- <y, w> (a double) in one pass (cmi_spmv_dia_dot_{f64,f32})."""
    import torch
    for t, n in ((values, "values"), (x, "x"), (y, "y"), (w, "w")):
        _need(t, n, y.dtype)
    _need(result, "result", torch.float64)
    _need(offsets, "offsets", torch.int32)
    if x.numel() != num_cols or y.numel() != num_rows or w.numel() != num_rows or offsets.numel() != num_diagonals or values.numel() < num_diagonals * pitch:
        raise ValueError("spmv_dia_dot: array lengths do not match the matrix shape")
    check(getattr(lib(), "cmi_spmv_dia_dot_" + _suffix(y))(num_rows, num_cols, num_diagonals, pitch, _ptr(offsets), _ptr(values), _ptr(x), _ptr(y),
                                                           _ptr(w), _ptr(result), _ptr(workspace), _cfg(cfg), _stream(stream)))


def spmv_coo(num_rows, num_cols, Ai, Aj, Ax, x, y, accumulate=False, cfg=None, stream=None):
    import torch
    for t, n in ((Ai, "Ai"), (Aj, "Aj")):
        _need(t, n, torch.int32)
    for t, n in ((Ax, "Ax"), (x, "x"), (y, "y")):
        _need(t, n, y.dtype)
    if Ai.numel() != Aj.numel() or Aj.numel() != Ax.numel() or x.numel() != num_cols or y.numel() != num_rows:
        raise ValueError("spmv_coo: array lengths do not match the matrix shape")
    fn = getattr(lib(), "cmi_spmv_coo_" + _suffix(y))
    check(fn(num_rows, num_cols, Ax.numel(), _ptr(Ai), _ptr(Aj), _ptr(Ax), _ptr(x), _ptr(y), int(bool(accumulate)),
             _cfg(cfg), _stream(stream)))


# ---- the semiring multiply (cmi_spmv_*_semiring_*): y[i] = the chain of row i under (combine, reduce), started from y0[i] or init ----
OP_PLUS, OP_MULTIPLIES, OP_MINIMUM, OP_MAXIMUM, OP_PROJECT1ST, OP_PROJECT2ND = range(6)
SEMIRING_OPS = {"plus": OP_PLUS, "multiplies": OP_MULTIPLIES, "minimum": OP_MINIMUM, "maximum": OP_MAXIMUM, "project1st": OP_PROJECT1ST,
                "project2nd": OP_PROJECT2ND}


def semiring_op(op):
    """cmi_op of a name ("plus", ..., "project2nd") or of an integer (handed on as it is: the library refuses what it does not know)."""
    if isinstance(op, str):
        if op not in SEMIRING_OPS:
            raise ValueError(f"unknown operation {op!r}: one of {sorted(SEMIRING_OPS)}")
        return SEMIRING_OPS[op]
    return int(op)


def _semiring_operands(who, y, index, values, x, y0, num_cols):
    """Checks shared by the four wrappers: tensors that may be None (streams the operations do not read), dtypes, the vectors' lengths."""
    import torch
    for t, n in index:
        _need(t, n, torch.int32)
    for t, n in (*values, (x, "x"), (y0, "y0"), (y, "y")):
        _need(t, n, y.dtype)
    if (x is not None and x.numel() != num_cols) or (y0 is not None and y0.numel() != y.numel()):
        raise ValueError(f"{who}: vector lengths do not match the matrix shape")


def spmv_csr_semiring(num_rows, num_cols, Ap, Aj, Ax, x, y, combine, reduce, y0=None, init=0.0, num_entries=None, stream=None):
    """cmi_spmv_csr_semiring_*.  Ax may be None with project2nd, Aj and x with project1st; y0=None starts every row from `init`."""
    _semiring_operands("spmv_csr_semiring", y, ((Ap, "Ap"), (Aj, "Aj")), ((Ax, "Ax"),), x, y0, num_cols)
    if Ap.numel() != num_rows + 1 or y.numel() != num_rows or (Aj is not None and Ax is not None and Aj.numel() != Ax.numel()):
        raise ValueError("spmv_csr_semiring: array lengths do not match the matrix shape")
    if num_entries is None:
        num_entries = (Aj if Aj is not None else Ax).numel()
    fn = getattr(lib(), "cmi_spmv_csr_semiring_" + _suffix(y))
    check(fn(num_rows, num_cols, num_entries, _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(x), _ptr(y0), float(init), semiring_op(combine), semiring_op(reduce),
             _ptr(y), _stream(stream)))


def spmv_coo_semiring(num_rows, num_cols, Ai, Aj, Ax, x, y, combine, reduce, y0=None, init=0.0, stream=None):
    """cmi_spmv_coo_semiring_*: entries sorted by row.  Ax may be None with project2nd, Aj and x with project1st."""
    _semiring_operands("spmv_coo_semiring", y, ((Ai, "Ai"), (Aj, "Aj")), ((Ax, "Ax"),), x, y0, num_cols)
    if y.numel() != num_rows or any(t is not None and t.numel() != Ai.numel() for t in (Aj, Ax)):
        raise ValueError("spmv_coo_semiring: array lengths do not match the matrix shape")
    fn = getattr(lib(), "cmi_spmv_coo_semiring_" + _suffix(y))
    check(fn(num_rows, num_cols, Ai.numel(), _ptr(Ai), _ptr(Aj), _ptr(Ax), _ptr(x), _ptr(y0), float(init), semiring_op(combine), semiring_op(reduce),
             _ptr(y), _stream(stream)))


def spmv_ell_semiring(num_rows, num_cols, width, pitch, Aj, Ax, x, y, combine, reduce, y0=None, init=0.0, stream=None):
    """cmi_spmv_ell_semiring_*: slots ascending, column -1 skipped.  Ax may be None with project2nd, x with project1st."""
    _semiring_operands("spmv_ell_semiring", y, ((Aj, "Aj"),), ((Ax, "Ax"),), x, y0, num_cols)
    if y.numel() != num_rows or any(t is not None and t.numel() < width * pitch for t in (Aj, Ax)):
        raise ValueError("spmv_ell_semiring: array lengths do not match the matrix shape")
    fn = getattr(lib(), "cmi_spmv_ell_semiring_" + _suffix(y))
    check(fn(num_rows, num_cols, width, pitch, _ptr(Aj), _ptr(Ax), _ptr(x), _ptr(y0), float(init), semiring_op(combine), semiring_op(reduce), _ptr(y),
             _stream(stream)))


def spmv_dia_semiring(num_rows, num_cols, num_diagonals, pitch, offsets, values, x, y, combine, reduce, y0=None, init=0.0, stream=None):
    """cmi_spmv_dia_semiring_*: every in-range slot takes part, stored zeros included.  values may be None with project2nd, x with project1st."""
    _semiring_operands("spmv_dia_semiring", y, ((offsets, "offsets"),), ((values, "values"),), x, y0, num_cols)
    if y.numel() != num_rows or offsets.numel() != num_diagonals or (values is not None and values.numel() < num_diagonals * pitch):
        raise ValueError("spmv_dia_semiring: array lengths do not match the matrix shape")
    fn = getattr(lib(), "cmi_spmv_dia_semiring_" + _suffix(y))
    check(fn(num_rows, num_cols, num_diagonals, pitch, _ptr(offsets), _ptr(values), _ptr(x), _ptr(y0), float(init), semiring_op(combine),
             semiring_op(reduce), _ptr(y), _stream(stream)))


def spmv_ell(num_rows, num_cols, width, pitch, Aj, Ax, x, y, row_lengths=None, accumulate=False, cfg=None,
             stream=None):
    import torch
    _need(Aj, "Aj", torch.int32)
    _need(row_lengths, "row_lengths", torch.int32)
    for t, n in ((Ax, "Ax"), (x, "x"), (y, "y")):
        _need(t, n, y.dtype)
    if Aj.numel() < width * pitch or Ax.numel() < width * pitch or x.numel() != num_cols or y.numel() != num_rows:
        raise ValueError("spmv_ell: array lengths do not match the matrix shape")
    fn = getattr(lib(), "cmi_spmv_ell_" + _suffix(y))
    check(fn(num_rows, num_cols, width, pitch, _ptr(Aj), _ptr(Ax), _ptr(row_lengths), _ptr(x), _ptr(y),
             int(bool(accumulate)), _cfg(cfg), _stream(stream)))


def spmv_dia(num_rows, num_cols, num_diagonals, pitch, offsets, values, x, y, accumulate=False, cfg=None,
             stream=None):
    import torch
    _need(offsets, "offsets", torch.int32)
    for t, n in ((values, "values"), (x, "x"), (y, "y")):
        _need(t, n, y.dtype)
    if offsets.numel() != num_diagonals or values.numel() < num_diagonals * pitch or x.numel() != num_cols \
            or y.numel() != num_rows:
        raise ValueError("spmv_dia: array lengths do not match the matrix shape")
    fn = getattr(lib(), "cmi_spmv_dia_" + _suffix(y))
    check(fn(num_rows, num_cols, num_diagonals, pitch, _ptr(offsets), _ptr(values), _ptr(x), _ptr(y),
             int(bool(accumulate)), _cfg(cfg), _stream(stream)))


def spmv_hyb(num_rows, num_cols, width, pitch, ell_Aj, ell_Ax, coo_Ai, coo_Aj, coo_Ax, x, y, accumulate=False,
             cfg_ell=None, cfg_coo=None, stream=None):
    import torch
    for t, n in ((ell_Aj, "ell_Aj"), (coo_Ai, "coo_Ai"), (coo_Aj, "coo_Aj")):
        _need(t, n, torch.int32)
    for t, n in ((ell_Ax, "ell_Ax"), (coo_Ax, "coo_Ax"), (x, "x"), (y, "y")):
        _need(t, n, y.dtype)
    fn = getattr(lib(), "cmi_spmv_hyb_" + _suffix(y))
    check(fn(num_rows, num_cols, width, pitch, _ptr(ell_Aj), _ptr(ell_Ax), coo_Ax.numel(), _ptr(coo_Ai), _ptr(coo_Aj),
             _ptr(coo_Ax), _ptr(x), _ptr(y), int(bool(accumulate)), _cfg(cfg_ell), _cfg(cfg_coo), _stream(stream)))


def hyb_plan_args(plan, pitch, ell_Aj, ell_Ax, coo_Ai, coo_Aj, coo_Ax):
    """Validate a HYB matrix's arrays against its plan ONCE and return what spmv_hyb_plan_args passes per call (a container
    that multiplies many times -- CG -- should not pay eight tensor checks per launch)."""
    import torch
    for t, n in ((ell_Aj, "ell_Aj"), (coo_Ai, "coo_Ai"), (coo_Aj, "coo_Aj")):
        _need(t, n, torch.int32)
    for t, n in ((ell_Ax, "ell_Ax"), (coo_Ax, "coo_Ax")):
        _need(t, n, ell_Ax.dtype)
    if plan.format != FORMAT_HYB:
        raise ValueError("hyb_plan_args: not a HYB plan")
    if (coo_Ai.numel() != plan.coo_entries or coo_Aj.numel() != plan.coo_entries or coo_Ax.numel() != plan.coo_entries
            or ell_Aj.numel() < plan.width * pitch or ell_Ax.numel() < plan.width * pitch or pitch < plan.num_rows):
        raise ValueError("hyb_plan_args: array lengths do not match the plan's matrix shape")
    return (getattr(lib(), "cmi_spmv_hyb_plan_" + _suffix(ell_Ax)), plan.handle, pitch, _ptr(ell_Aj), _ptr(ell_Ax), _ptr(coo_Ai), _ptr(coo_Aj),
            _ptr(coo_Ax), ell_Ax.dtype, plan.num_cols, plan.num_rows)


def spmv_hyb_plan_args(args, x, y, accumulate=False, stream=None):
    fn, h, pitch, eAj, eAx, cAi, cAj, cAx, dt, ncols, nrows = args
    if x.dtype != dt or y.dtype != dt or not x.is_cuda or not y.is_cuda or x.numel() != ncols or y.numel() != nrows \
            or not x.is_contiguous() or not y.is_contiguous():
        raise ValueError("spmv_hyb_plan: x / y must be contiguous device vectors of the matrix's value type and shape")
    check(fn(h, pitch, eAj, eAx, cAi, cAj, cAx, _ptr(x), _ptr(y), int(bool(accumulate)), _stream(stream)))


def spmv_coo_dot_plan(plan, Ai, Aj, Ax, x, y, w, result, workspace, stream=None):
    """cmi_spmv_coo_dot_plan_*: y <- A x and result[0] <- <y, w> (a double); one pass for sorted entries (the plan's row offsets)."""
    import torch
    for t, n in ((Ai, "Ai"), (Aj, "Aj")):
        _need(t, n, torch.int32)
    for t, n in ((Ax, "Ax"), (x, "x"), (y, "y"), (w, "w")):
        _need(t, n, y.dtype)
    _need(result, "result", torch.float64)
    if (Ai.numel() != plan.num_entries or Aj.numel() != plan.num_entries or Ax.numel() != plan.num_entries
            or x.numel() != plan.num_cols or y.numel() != plan.num_rows or w.numel() != plan.num_rows):
        raise ValueError("spmv_coo_dot_plan: array lengths do not match the plan's matrix shape")
    check(getattr(lib(), "cmi_spmv_coo_dot_plan_" + _suffix(y))(plan.handle, _ptr(Ai), _ptr(Aj), _ptr(Ax), _ptr(x), _ptr(y), _ptr(w), _ptr(result),
                                                                _ptr(workspace), _stream(stream)))


def spmv_hyb_dot_plan_args(args, x, y, w, result, workspace, stream=None):
    """cmi_spmv_hyb_dot_plan_*: y <- A x and result[0] <- <y, w> (a double), one pass where the plan runs one launch."""
    import torch
    fn, h, pitch, eAj, eAx, cAi, cAj, cAx, dt, ncols, nrows = args
    if x.dtype != dt or y.dtype != dt or w.dtype != dt or x.numel() != ncols or y.numel() != nrows or w.numel() != nrows:
        raise ValueError("spmv_hyb_dot_plan: x / y / w must be device vectors of the matrix's value type and shape")
    _need(result, "result", torch.float64)
    fnd = getattr(lib(), "cmi_spmv_hyb_dot_plan_" + _suffix(y))
    check(fnd(h, pitch, eAj, eAx, cAi, cAj, cAx, _ptr(x), _ptr(y), _ptr(w), _ptr(result), _ptr(workspace), _stream(stream)))


def set_index_compression(on):
    """cmi_set_index_compression: every later AUTO-kernel plan of Plan.csr / CsrMatrix tries the 16-bit column copy."""
    check(lib().cmi_set_index_compression(int(bool(on))))


def get_index_compression():
    return bool(lib().cmi_get_index_compression())


def plan_set_row_scale(plan, scale):
    """cmi_plan_set_row_scale: every later multiply through the one-launch HYB plan stores y[i] = (A x)[i] * scale[i] (one more multiply, rounded
    on its own: the bits of spmv_hyb_plan followed by blas_xmy); None clears it.  The plan keeps the pointer: `scale` (num_rows device values of
    the plan's type) is held by the Plan object so that it outlives the multiplies, and its values may be changed in place.  CmiError
    NOT_SUPPORTED for any plan that is not a HYB plan with hyb_launches() == 1, INVALID_VALUE for plan None."""
    import torch
    if plan is not None and scale is not None:
        want = torch.float64 if plan.dtype == F64 else torch.float32
        if not scale.is_cuda or scale.dtype != want or scale.numel() != plan.num_rows or not scale.is_contiguous():
            raise ValueError("plan_set_row_scale: scale must be a contiguous device vector of num_rows values of the plan's value type")
    check(lib().cmi_plan_set_row_scale(None if plan is None else plan.handle, _ptr(scale)))
    if plan is not None:
        plan._row_scale = scale


def plan_drop_const_tiles(plan):
    """cmi_plan_drop_const_tiles (no stream: it launches nothing).  CmiError INVALID_VALUE for plan None."""
    check(lib().cmi_plan_drop_const_tiles(None if plan is None else plan.handle))


def spmv_hyb_plan(plan, pitch, ell_Aj, ell_Ax, coo_Ai, coo_Aj, coo_Ax, x, y, accumulate=False, stream=None):
    """cmi_spmv_hyb_plan_*: one launch when the plan found the COO part sorted by row (storage-order sums, y written once)."""
    import torch
    for t, n in ((ell_Aj, "ell_Aj"), (coo_Ai, "coo_Ai"), (coo_Aj, "coo_Aj")):
        _need(t, n, torch.int32)
    for t, n in ((ell_Ax, "ell_Ax"), (coo_Ax, "coo_Ax"), (x, "x"), (y, "y")):
        _need(t, n, y.dtype)
    if plan.format != FORMAT_HYB:
        raise ValueError("spmv_hyb_plan: not a HYB plan")
    if (coo_Ai.numel() != plan.coo_entries or coo_Aj.numel() != plan.coo_entries or coo_Ax.numel() != plan.coo_entries
            or ell_Aj.numel() < plan.width * pitch or ell_Ax.numel() < plan.width * pitch or pitch < plan.num_rows
            or x.numel() != plan.num_cols or y.numel() != plan.num_rows):
        raise ValueError("spmv_hyb_plan: array lengths do not match the plan's matrix shape")
    fn = getattr(lib(), "cmi_spmv_hyb_plan_" + _suffix(y))
    check(fn(plan.handle, pitch, _ptr(ell_Aj), _ptr(ell_Ax), _ptr(coo_Ai), _ptr(coo_Aj), _ptr(coo_Ax), _ptr(x), _ptr(y),
             int(bool(accumulate)), _stream(stream)))


# ------------------------------------------------------------------------------------------------
# tuning table
# ------------------------------------------------------------------------------------------------
def tuning_select(fmt, dtype, num_rows, num_cols, num_entries):
    c = Config()
    check(lib().cmi_tuning_select(fmt, dtype, num_rows, num_cols, num_entries, ctypes.byref(c)))
    return c


HYB_RULE_REFERENCE, HYB_RULE_COST, HYB_RULE_COST2 = 0, 1, 2


def count_zeros(values, stream=None):
    """explicit zeros in a device value array (cmi_count_zeros_*: the reference's ELL num_entries excludes them)"""
    c = c_int64()
    check(getattr(lib(), "cmi_count_zeros_" + _suffix(values))(values.numel(), _ptr(values), byref(c), _stream(stream)))
    return c.value


def tuning_hyb_rule(dtype):
    """(kind, relative_speed, threshold) of the HYB split rule for F64 / F32; without a table the reference's
    (HYB_RULE_REFERENCE, 3.0, 4096)."""
    k, rs, th = c_int(), c_double(), c_int64()
    check(lib().cmi_tuning_hyb_rule(dtype, byref(k), byref(rs), byref(th)))
    return k.value, rs.value, th.value


def tuning_waver_rule(dtype):
    """csr_waver's launch shape and AUTO gates for F64 / F32 (cmi_waver_rule): the table's "waver_rule", else the built-in one."""
    r = WaverRule()
    check(lib().cmi_tuning_waver_rule(dtype, byref(r)))
    return r


def tuning_set_waver_rule(dtype, items_per_thread=4, cap=0, xcd_swizzle=16, min_piece=None, min_entries=None):
    """layer a csr_waver rule on the table (tools/autotune_waver.py writes it; tuning_save persists it)"""
    r = WaverRule(int(items_per_thread), int(cap), int(xcd_swizzle), 0, float((2.2 if dtype == F64 else 1.9) if min_piece is None else min_piece),
                  int((4_400_000 if dtype == F64 else 6_400_000) if min_entries is None else min_entries))
    check(lib().cmi_tuning_set_waver_rule(dtype, byref(r)))


def tuning_hyb_light_speed(dtype):
    """HYB_RULE_COST2's fourth parameter: cost of a COO entry (ELL slots) while the COO part is light enough for one launch."""
    v = c_double()
    check(lib().cmi_tuning_hyb_light_speed(dtype, byref(v)))
    return v.value


def tuning_set_hyb_light_speed(dtype, light_speed):
    check(lib().cmi_tuning_set_hyb_light_speed(dtype, float(light_speed)))


def tuning_set_hyb_rule(dtype, kind, relative_speed, threshold):
    check(lib().cmi_tuning_set_hyb_rule(dtype, int(kind), float(relative_speed), int(threshold)))


def hyb_entries_per_row(dtype, num_rows, Ap, kind=-1, relative_speed=0.0, threshold=0, stream=None):
    """ELL width of the HYB split for the CSR matrix with row offsets Ap (device): the tuned rule (kind < 0), or an explicit
    rule -- (HYB_RULE_REFERENCE, 3.0, 4096) reproduces the reference's widths."""
    import torch
    _need(Ap, "Ap", torch.int32)
    code = F64 if dtype in (F64, torch.float64) else F32
    w = c_int64()
    check(lib().cmi_hyb_entries_per_row(code, num_rows, _ptr(Ap), int(kind), float(relative_speed), int(threshold), byref(w),
                                        _stream(stream)))
    return w.value


def tuning_set(fmt, dtype, mean_entries_per_row, cfg):
    check(lib().cmi_tuning_set(fmt, dtype, float(mean_entries_per_row), ctypes.byref(cfg)))


def tuning_load(path):
    check(lib().cmi_tuning_load(path.encode() if path else None))


def tuning_save(path):
    check(lib().cmi_tuning_save(path.encode()))


def tuning_clear():
    check(lib().cmi_tuning_clear())


# ------------------------------------------------------------------------------------------------
# on-device builders
# ------------------------------------------------------------------------------------------------
def poisson5pt_num_entries(m, n):
    return int(lib().cmi_poisson5pt_num_entries(m, n))


def poisson5pt_shard_entries(m, n, row_begin, row_end):
    return int(lib().cmi_poisson5pt_shard_entries(m, n, row_begin, row_end))


def poisson5pt_csr(m, n, Ap, Aj, Ax, row_begin=0, row_end=None, stream=None):
    import torch
    row_end = m * n if row_end is None else row_end
    _need(Ap, "Ap", torch.int32)
    _need(Aj, "Aj", torch.int32)
    _need(Ax, "Ax")
    nnz = poisson5pt_shard_entries(m, n, row_begin, row_end)
    if Ap.numel() != row_end - row_begin + 1 or Aj.numel() < nnz or Ax.numel() < nnz:
        raise ValueError("poisson5pt_csr: output arrays too small")
    fn = getattr(lib(), "cmi_poisson5pt_csr_" + _suffix(Ax))
    check(fn(m, n, row_begin, row_end, _ptr(Ap), _ptr(Aj), _ptr(Ax), _stream(stream)))


def poisson5pt_dia(m, n, pitch, offsets, values, stream=None):
    import torch
    _need(offsets, "offsets", torch.int32)
    _need(values, "values")
    if offsets.numel() != 5 or values.numel() < 5 * pitch:
        raise ValueError("poisson5pt_dia: output arrays too small")
    fn = getattr(lib(), "cmi_poisson5pt_dia_" + _suffix(values))
    check(fn(m, n, pitch, _ptr(offsets), _ptr(values), _stream(stream)))


def csr_to_ell(num_rows, Ap, Aj, Ax, width, pitch, ell_Aj, ell_Ax, stream=None):
    import torch
    for t, n in ((Ap, "Ap"), (Aj, "Aj"), (ell_Aj, "ell_Aj")):
        _need(t, n, torch.int32)
    _need(Ax, "Ax", ell_Ax.dtype)
    _need(ell_Ax, "ell_Ax")
    if ell_Aj.numel() < width * pitch or ell_Ax.numel() < width * pitch:
        raise ValueError("csr_to_ell: output arrays too small")
    fn = getattr(lib(), "cmi_csr_to_ell_" + _suffix(ell_Ax))
    check(fn(num_rows, _ptr(Ap), _ptr(Aj), _ptr(Ax), width, pitch, _ptr(ell_Aj), _ptr(ell_Ax), _stream(stream)))


def csr_to_hyb_coo(num_rows, Ap, Aj, Ax, width, coo_offsets, coo_Ai, coo_Aj, coo_Ax, stream=None):
    import torch
    for t, n in ((Ap, "Ap"), (Aj, "Aj"), (coo_offsets, "coo_offsets"), (coo_Ai, "coo_Ai"), (coo_Aj, "coo_Aj")):
        _need(t, n, torch.int32)
    _need(Ax, "Ax", coo_Ax.dtype)
    _need(coo_Ax, "coo_Ax")
    fn = getattr(lib(), "cmi_csr_to_hyb_coo_" + _suffix(coo_Ax))
    check(fn(num_rows, _ptr(Ap), _ptr(Aj), _ptr(Ax), width, _ptr(coo_offsets), _ptr(coo_Ai), _ptr(coo_Aj), _ptr(coo_Ax),
             _stream(stream)))


def csr_diagonals(num_rows, num_cols, Ap, Aj, slot_map, diag_list, stream=None):
    """Flags the occupied diagonals in slot_map, lists their offsets (unordered) in diag_list; returns the
    count (may exceed diag_list.numel(): list truncated).  Synchronises."""
    n = c_int64()
    check(lib().cmi_csr_diagonals(num_rows, num_cols, _ptr(Ap), _ptr(Aj), _ptr(slot_map), _ptr(diag_list), diag_list.numel(),
                                  byref(n), _stream(stream)))
    return n.value


def csr_to_dia(num_rows, num_cols, Ap, Aj, Ax, offsets, pitch, slot_map, values, stream=None):
    check(getattr(lib(), "cmi_csr_to_dia_" + _suffix(Ax))(num_rows, num_cols, _ptr(Ap), _ptr(Aj), _ptr(Ax), offsets.numel(), pitch,
                                                         _ptr(offsets), _ptr(slot_map), _ptr(values), _stream(stream)))


def csr_row_indices(num_rows, Ap, Ai, stream=None):
    import torch
    _need(Ap, "Ap", torch.int32)
    _need(Ai, "Ai", torch.int32)
    check(lib().cmi_csr_row_indices(num_rows, _ptr(Ap), _ptr(Ai), _stream(stream)))


def ell_row_lengths(num_rows, width, pitch, ell_Aj, row_lengths, stream=None):
    import torch
    _need(ell_Aj, "ell_Aj", torch.int32)
    _need(row_lengths, "row_lengths", torch.int32)
    check(lib().cmi_ell_row_lengths(num_rows, width, pitch, _ptr(ell_Aj), _ptr(row_lengths), _stream(stream)))


# ------------------------------------------------------------------------------------------------
# BLAS-1 (f64)
# ------------------------------------------------------------------------------------------------
def blas_workspace(device="cuda"):
    import torch
    return torch.empty(lib().cmi_blas_workspace_bytes() // 8, dtype=torch.float64, device=device)


def blas_axpy(alpha, x, y, stream=None):
    check(getattr(lib(), "cmi_blas_axpy_" + _suffix(y))(x.numel(), float(alpha), _ptr(x), _ptr(y), _stream(stream)))


def blas_axpby(alpha, x, beta, y, z, stream=None):
    check(getattr(lib(), "cmi_blas_axpby_" + _suffix(z))(x.numel(), float(alpha), _ptr(x), float(beta), _ptr(y), _ptr(z),
                                                      _stream(stream)))


def blas_copy(x, y, stream=None):
    check(getattr(lib(), "cmi_blas_copy_" + _suffix(y))(x.numel(), _ptr(x), _ptr(y), _stream(stream)))


def blas_fill(value, y, stream=None):
    check(getattr(lib(), "cmi_blas_fill_" + _suffix(y))(y.numel(), float(value), _ptr(y), _stream(stream)))


def blas_dot(x, y, result, workspace, stream=None):
    """result: 1-element device tensor of x's dtype."""
    check(getattr(lib(), "cmi_blas_dot_" + _suffix(x))(x.numel(), _ptr(x), _ptr(y), _ptr(result), _ptr(workspace),
                                                    _stream(stream)))


def blas_nrm2(x, result, workspace, stream=None):
    check(getattr(lib(), "cmi_blas_nrm2_" + _suffix(x))(x.numel(), _ptr(x), _ptr(result), _ptr(workspace), _stream(stream)))


def cg_update(rz, yp, p, y, x, r, rr_out, workspace, stream=None, mirror=None):
    """alpha = rz/yp (device scalars); x += alpha p (x None: left to cg_direction_x); r -= alpha y; rr_out = <r, r> -- one pass.
    mirror: a HostScalar that also receives <r, r> (no copy); its event is recorded behind the call."""
    check(getattr(lib(), "cmi_cg_update_" + _suffix(r))(r.numel(), _ptr(rz), _ptr(yp), _ptr(p) if x is not None else None, _ptr(y),
                                  _ptr(x) if x is not None else None, _ptr(r), _ptr(rr_out),
                                  mirror.ptr if mirror is not None else None, _ptr(workspace), _stream(stream)))
    if mirror is not None:
        mirror.record(stream)


def spmv_csr_dot_partials(plan, Ap, Aj, Ax, x, y, w, workspace, stream=None):
    """cmi_spmv_csr_dot_plan_partials_*: y <- A x, the per-tile partials of <y, w> left in the workspace for cg_update_fold.
    Returns their count (0: this plan's kernel cannot fuse the dot)."""
    n = c_int()
    check(getattr(lib(), "cmi_spmv_csr_dot_plan_partials_" + _suffix(y))(plan.handle, _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(x), _ptr(y), _ptr(w),
                                                                         _ptr(workspace), byref(n), _stream(stream)))
    return n.value


def cg_update_fold(rz, yp_out, npartials_yp, y, r, workspace, stream=None):
    """cmi_cg_update_fold_*: yp <- fold of the workspace's <y, p> partials (also stored to yp_out); r -= (rz/yp) y; returns the
    number of <r, r> partials left in the workspace's second area."""
    n = c_int()
    check(getattr(lib(), "cmi_cg_update_fold_" + _suffix(r))(r.numel(), _ptr(rz), _ptr(yp_out), int(npartials_yp), _ptr(y), _ptr(r),
                                                             _ptr(workspace), byref(n), _stream(stream)))
    return n.value


def cg_direction_x_fold(rr_new_out, npartials_rr, rr_old, yp, r, p, x, workspace, stream=None, mirror=None):
    """cmi_cg_direction_x_fold_*: rr_new <- fold of the <r, r> partials (stored to rr_new_out and the HostScalar `mirror`);
    x += (rr_old/yp) p; p = r + (rr_new/rr_old) p."""
    check(getattr(lib(), "cmi_cg_direction_x_fold_" + _suffix(r))(r.numel(), _ptr(rr_new_out), mirror.ptr if mirror is not None else None,
                                                                  int(npartials_rr), _ptr(rr_old), _ptr(yp), _ptr(r), _ptr(p), _ptr(x),
                                                                  _ptr(workspace), _stream(stream)))
    if mirror is not None:
        mirror.record(stream)


# ------------------------------------------------------------------------------------------------
# the rest of BLAS-1 and the fused solver steps (csrc/blas1_extra.hip).  Scalars named rz, yp, rho, d1, ... and every
# reduction result are 1-element float64 device tensors whatever the vectors' dtype; `mirror` is a HostScalar.
# ------------------------------------------------------------------------------------------------
def _mirror(mirror):
    return mirror.ptr if mirror is not None else None


def blas_scal(alpha, x, stream=None):
    """x <- alpha x."""
    check(getattr(lib(), "cmi_blas_scal_" + _suffix(x))(x.numel(), float(alpha), _ptr(x), _stream(stream)))


def blas_xmy(x, y, z, stream=None):
    """z <- x .* y (z may be x or y)."""
    check(getattr(lib(), "cmi_blas_xmy_" + _suffix(z))(x.numel(), _ptr(x), _ptr(y), _ptr(z), _stream(stream)))


def blas_axpbypcz(alpha, x, beta, y, gamma, z, out, stream=None):
    """out <- (alpha x + beta y) + gamma z."""
    check(getattr(lib(), "cmi_blas_axpbypcz_" + _suffix(out))(x.numel(), float(alpha), _ptr(x), float(beta), _ptr(y), float(gamma), _ptr(z),
                                                               _ptr(out), _stream(stream)))


def blas_asum(x, result, workspace, stream=None):
    """result (1 element of x's dtype) <- sum |x_i|."""
    check(getattr(lib(), "cmi_blas_asum_" + _suffix(x))(x.numel(), _ptr(x), _ptr(result), _ptr(workspace), _stream(stream)))


def blas_amax(x, value, index, workspace, stream=None):
    """value (1 element of x's dtype) <- max |x_i|, index (1 int64) <- its first position; either may be None."""
    check(getattr(lib(), "cmi_blas_amax_" + _suffix(x))(x.numel(), _ptr(x), _ptr(value), _ptr(index), _ptr(workspace), _stream(stream)))


def pcg_update_jacobi(rz, yp, y, r, dinv, rz_new, rr, workspace, stream=None, mirror=None):
    """alpha = rz/yp; r -= alpha y; rz_new = <r, dinv r>; rr = <r, r> (also to `mirror`)."""
    check(getattr(lib(), "cmi_pcg_update_jacobi_" + _suffix(r))(r.numel(), _ptr(rz), _ptr(yp), _ptr(y), _ptr(r), _ptr(dinv), _ptr(rz_new), _ptr(rr),
                                                                 _mirror(mirror), _ptr(workspace), _stream(stream)))
    if mirror is not None:
        mirror.record(stream)


def pcg_direction_x_jacobi(rz_new, rz_old, yp, r, dinv, p, x, stream=None):
    """x += (rz_old/yp) p; p = dinv r + (rz_new/rz_old) p."""
    check(getattr(lib(), "cmi_pcg_direction_x_jacobi_" + _suffix(r))(r.numel(), _ptr(rz_new), _ptr(rz_old), _ptr(yp), _ptr(r), _ptr(dinv), _ptr(p),
                                                                      _ptr(x), _stream(stream)))


def bicgstab_s(rho, d1, r, AMp, s, ss, workspace, stream=None, mirror=None):
    """alpha = rho/d1; s = r - alpha AMp; ss = <s, s> (also to `mirror`)."""
    check(getattr(lib(), "cmi_bicgstab_s_" + _suffix(s))(s.numel(), _ptr(rho), _ptr(d1), _ptr(r), _ptr(AMp), _ptr(s), _ptr(ss), _mirror(mirror),
                                                          _ptr(workspace), _stream(stream)))
    if mirror is not None:
        mirror.record(stream)


def bicgstab_xr(rho, d1, d2, d3, p, s, AMs, r_star, x, r, rho_new, rr, workspace, stream=None, mirror=None):
    """alpha = rho/d1, omega = d2/d3; x += alpha p + omega s; r = s - omega AMs; rho_new = <r_star, r>; rr = <r, r> (also to `mirror`)."""
    check(getattr(lib(), "cmi_bicgstab_xr_" + _suffix(r))(r.numel(), _ptr(rho), _ptr(d1), _ptr(d2), _ptr(d3), _ptr(p), _ptr(s), _ptr(AMs), _ptr(r_star),
                                                           _ptr(x), _ptr(r), _ptr(rho_new), _ptr(rr), _mirror(mirror), _ptr(workspace), _stream(stream)))
    if mirror is not None:
        mirror.record(stream)


def bicgstab_p(rho_new, rho, d1, d2, d3, r, AMp, p, stream=None):
    """beta = (rho_new/rho) (alpha/omega); p = r + beta (p - omega AMp)."""
    check(getattr(lib(), "cmi_bicgstab_p_" + _suffix(p))(p.numel(), _ptr(rho_new), _ptr(rho), _ptr(d1), _ptr(d2), _ptr(d3), _ptr(r), _ptr(AMp), _ptr(p),
                                                          _stream(stream)))


# the multi-shift solver steps (csrc/krylov_m.hip): x, p_s and s_s hold shift s at [s ld, s ld + n); sigma and the per-shift coefficient
# tensors hold num_shifts values of the vectors' dtype
def _need_all(who, dtype, **tensors):
    for name, t in tensors.items():
        _need(t, f"{who}: {name}", dtype)


def cg_m_coefficients(rsq_old, pAp, rsq_new, state, sigma, zeta_m1, zeta_0, beta_s, alpha_s, stream=None):
    """beta_0 = -(rsq_old/pAp), alpha_0 = rsq_new/rsq_old (1-element float64 device tensors); per shift: the next zeta (clamped) and beta_s from
    (state = previous (beta_0, alpha_0), zeta_m1, zeta_0, sigma), alpha_s, the rotation of zeta; then state <- (beta_0, alpha_0)."""
    import torch
    _need_all("cg_m_coefficients", torch.float64, rsq_old=rsq_old, pAp=pAp, rsq_new=rsq_new)
    _need_all("cg_m_coefficients", state.dtype, state=state, sigma=sigma, zeta_m1=zeta_m1, zeta_0=zeta_0, beta_s=beta_s, alpha_s=alpha_s)
    check(getattr(lib(), "cmi_cg_m_coefficients_" + _suffix(state))(sigma.numel(), _ptr(rsq_old), _ptr(pAp), _ptr(rsq_new), _ptr(state), _ptr(sigma), _ptr(zeta_m1),
                                                                     _ptr(zeta_0), _ptr(beta_s), _ptr(alpha_s), _stream(stream)))


def cg_m_update_xp(n, ld, state, beta_s, alpha_s, zeta_0, r, p0, x, p_s, stream=None):
    """p0 <- r + state[1] p0 (p0 None: skipped); per shift x_s <- x_s - beta_s p_s (the old p_s), p_s <- zeta_0[s] r + alpha_s p_s."""
    _need_all("cg_m_update_xp", r.dtype, state=state, beta_s=beta_s, alpha_s=alpha_s, zeta_0=zeta_0, r=r, p0=p0, x=x, p_s=p_s)
    check(getattr(lib(), "cmi_cg_m_update_xp_" + _suffix(r))(int(n), beta_s.numel(), int(ld), _ptr(state), _ptr(beta_s), _ptr(alpha_s), _ptr(zeta_0), _ptr(r),
                                                              _ptr(p0), _ptr(x), _ptr(p_s), _stream(stream)))


def _ptr_given(t, stand_in):
    """_ptr for an operand whose PRESENCE selects a form of the call: an empty tensor has no address, so it hands over `stand_in`'s (never
    dereferenced: the call has n == 0)."""
    return None if t is None else c_void_p(t.data_ptr() or stand_in.data_ptr())


def lobpcg_residual(lambda_dev, x, ax, r, rr_out, workspace, stream=None, mirror=None):
    """r <- T(-lambda) x + ax (lambda: a 1-element float64 device tensor); rr_out <- <r, r>, also to the HostScalar `mirror`."""
    import torch
    _need_all("lobpcg_residual", torch.float64, lambda_dev=lambda_dev, rr_out=rr_out, workspace=workspace)
    _need_all("lobpcg_residual", r.dtype, x=x, ax=ax, r=r)
    check(getattr(lib(), "cmi_lobpcg_residual_" + _suffix(r))(r.numel(), _ptr(lambda_dev), _ptr(x), _ptr(ax), _ptr(r), _ptr(rr_out),
                                                               mirror.ptr if mirror is not None else None, _ptr(workspace), _stream(stream)))
    if mirror is not None:
        mirror.record(stream)


def lobpcg_gram(pp, x, w, aw, p, ap, gram_out, workspace, stream=None):
    """p, ap <- s p, s ap with s = T(1) / T(sqrt(pp)) (pp: 1 float64 on the device), and from the scaled values gram_out[0..7] = <x,aw>, <w,aw>,
    <x,w>, <x,ap>, <w,ap>, <p,ap>, <x,p>, <w,p> (float64).  p and ap None (the first iteration): only gram_out[0..2]; pp may be None."""
    import torch
    _need_all("lobpcg_gram", torch.float64, pp=pp, gram_out=gram_out, workspace=workspace)
    _need_all("lobpcg_gram", x.dtype, x=x, w=w, aw=aw, p=p, ap=ap)
    check(getattr(lib(), "cmi_lobpcg_gram_" + _suffix(x))(x.numel(), _ptr(pp), _ptr(x), _ptr(w), _ptr(aw), _ptr_given(p, gram_out), _ptr_given(ap, gram_out), _ptr(gram_out),
                                                           _ptr(workspace),
                                                           _stream(stream)))


def lobpcg_update(cx, cr, cp, first, lambda_new, w, aw, p, ap, x, ax, r, scalars_out, workspace, stream=None, mirror=None):
    """p, ap <- cr (w, aw) + cp (p, ap) (first: cr (w, aw) + (p, ap)); x, ax <- cx (x, ax) + (p, ap); r <- T(-lambda_new) x + ax (r None: skipped);
    scalars_out[0] <- <r, r> (also to `mirror`), scalars_out[1] <- <p, p>.  The scalars by value."""
    import torch
    _need_all("lobpcg_update", torch.float64, scalars_out=scalars_out, workspace=workspace)
    _need_all("lobpcg_update", x.dtype, w=w, aw=aw, p=p, ap=ap, x=x, ax=ax, r=r)
    use_mirror = mirror is not None and r is not None
    check(getattr(lib(), "cmi_lobpcg_update_" + _suffix(x))(x.numel(), float(cx), float(cr), float(cp), int(bool(first)), float(lambda_new), _ptr(w), _ptr(aw),
                                                             _ptr(p), _ptr(ap), _ptr(x), _ptr(ax), _ptr_given(r, scalars_out), _ptr(scalars_out),
                                                             mirror.ptr if use_mirror else None, _ptr(workspace), _stream(stream)))
    if use_mirror:
        mirror.record(stream)


def dense_gemm(m, n, k, A, lda, B, ldb, C, ldc, stream=None):
    """C (m x n) <- A (m x k) B (k x n), column-major with leading dimensions lda, ldb, ldc: A, B and C are 1-D device tensors of one dtype that
    hold the operands from their first element (views at any element offset); the chain of each element starts at +0 and adds j ascending."""
    _need_all("dense_gemm", C.dtype, A=A, B=B, C=C)
    check(getattr(lib(), "cmi_dense_gemm_" + _suffix(C))(int(m), int(n), int(k), _ptr(A), int(lda), _ptr(B), int(ldb), _ptr(C), int(ldc), _stream(stream)))


def bicgstab_m_s(alpha_1, chi_0, r_1, As, s_0, stream=None):
    """s_0 <- r_1 + alpha_1 (s_0 - chi_0 As); the scalars by value."""
    _need_all("bicgstab_m_s", s_0.dtype, r_1=r_1, As=As, s_0=s_0)
    check(getattr(lib(), "cmi_bicgstab_m_s_" + _suffix(s_0))(s_0.numel(), float(alpha_1), float(chi_0), _ptr(r_1), _ptr(As), _ptr(s_0), _stream(stream)))


def bicgstab_m_coefficients(beta_m1, beta_0, alpha_old, alpha_new, chi_0, sigma, zeta_m1, zeta_0, rho_0, zeta_1, beta_s, chi_s, rho_1, alpha_s, stream=None):
    """Per shift: zeta_1 (clamped) and beta_s from the old alpha, chi_s and rho_1, alpha_s from the new alpha; nothing rotates."""
    _need_all("bicgstab_m_coefficients", sigma.dtype, sigma=sigma, zeta_m1=zeta_m1, zeta_0=zeta_0, rho_0=rho_0, zeta_1=zeta_1, beta_s=beta_s, chi_s=chi_s,
              rho_1=rho_1, alpha_s=alpha_s)
    check(getattr(lib(), "cmi_bicgstab_m_coefficients_" + _suffix(sigma))(sigma.numel(), float(beta_m1), float(beta_0), float(alpha_old), float(alpha_new),
                                                                           float(chi_0), _ptr(sigma), _ptr(zeta_m1), _ptr(zeta_0), _ptr(rho_0), _ptr(zeta_1),
                                                                           _ptr(beta_s), _ptr(chi_s), _ptr(rho_1), _ptr(alpha_s), _stream(stream)))


def bicgstab_m_update_xs(n, ld, beta_s, chi_s, rho_0, zeta_m1, zeta_0, alpha_s, rho_1, zeta_1, r_0, r_1, w_1, x, s_s, stream=None):
    """Per shift x_s and s_s (KERNEL_XS), then the rotation zeta_m1 <- zeta_0 <- zeta_1, rho_0 <- rho_1 (a tail launch of the same call)."""
    _need_all("bicgstab_m_update_xs", x.dtype, beta_s=beta_s, chi_s=chi_s, rho_0=rho_0, zeta_m1=zeta_m1, zeta_0=zeta_0, alpha_s=alpha_s, rho_1=rho_1, zeta_1=zeta_1,
              r_0=r_0, r_1=r_1, w_1=w_1, x=x, s_s=s_s)
    check(getattr(lib(), "cmi_bicgstab_m_update_xs_" + _suffix(x))(int(n), beta_s.numel(), int(ld), _ptr(beta_s), _ptr(chi_s), _ptr(rho_0), _ptr(zeta_m1), _ptr(zeta_0),
                                                                    _ptr(alpha_s), _ptr(rho_1), _ptr(zeta_1), _ptr(r_0), _ptr(r_1), _ptr(w_1), _ptr(x), _ptr(s_s),
                                                                    _stream(stream)))


def cr_xr(rz, yy, p, y, x, r, rr, workspace, update_r=True, stream=None, mirror=None):
    """alpha = rz/yy; x += alpha p; with update_r also r -= alpha y and rr = <r, r> (also to `mirror`)."""
    check(getattr(lib(), "cmi_cr_xr_" + _suffix(x))(x.numel(), _ptr(rz), _ptr(yy), _ptr(p), _ptr(y), _ptr(x), _ptr(r), int(bool(update_r)), _ptr(rr),
                                                     _mirror(mirror), _ptr(workspace), _stream(stream)))
    if mirror is not None and update_r:
        mirror.record(stream)


def cr_py(rz_new, rz, r, Ar, p, y, yy_new, workspace, stream=None):
    """beta = rz_new/rz; p = r + beta p; y = Ar + beta y; yy_new = <y, y>."""
    check(getattr(lib(), "cmi_cr_py_" + _suffix(p))(p.numel(), _ptr(rz_new), _ptr(rz), _ptr(r), _ptr(Ar), _ptr(p), _ptr(y), _ptr(yy_new), _ptr(workspace),
                                                     _stream(stream)))


def blas_axpy_dot(h, v, w, u, out, workspace, stream=None):
    """w -= (*h) v; out = <w, u> (u may be w: the norm's square).  h None: the dot alone, v unused."""
    check(getattr(lib(), "cmi_blas_axpy_dot_" + _suffix(w))(w.numel(), _ptr(h), _ptr(v), _ptr(w), _ptr(u), _ptr(out), _ptr(workspace), _stream(stream)))


def blas_axpy_ratio(num, den, x, y, stream=None):
    """y += (num/den) x."""
    check(getattr(lib(), "cmi_blas_axpy_ratio_" + _suffix(y))(y.numel(), _ptr(num), _ptr(den), _ptr(x), _ptr(y), _stream(stream)))


def csr_diagonal(num_rows, Ap, Aj, Ax, diag, reciprocal=False, stream=None):
    """diag[i] <- the sum of row i's entries in column i, or its reciprocal."""
    check(getattr(lib(), "cmi_csr_diagonal_" + _suffix(diag))(num_rows, _ptr(Ap), _ptr(Aj), _ptr(Ax), _ptr(diag), int(bool(reciprocal)), _stream(stream)))


# ------------------------------------------------------------------------------------------------
# cusp::eigen's kernels (csrc/eigen.hip): absolute row sums per format, the start vector, the normalise step
# ------------------------------------------------------------------------------------------------
def csr_abs_row_sums(num_rows, Ap, Ax, row_sums, accumulate=False, stream=None):
    """row_sums[i] (+)= sum of |Ax[Ap[i] .. Ap[i + 1])|: reads the row offsets and the values, never the columns."""
    import torch
    _need(Ap, "Ap", torch.int32)
    _need(Ax, "Ax", row_sums.dtype)
    _need(row_sums, "row_sums")
    if Ap.numel() < num_rows + 1 or row_sums.numel() < num_rows:
        raise ValueError("csr_abs_row_sums: array lengths do not match num_rows")
    check(getattr(lib(), "cmi_csr_abs_row_sums_" + _suffix(row_sums))(num_rows, _ptr(Ap), _ptr(Ax), _ptr(row_sums), int(bool(accumulate)), _stream(stream)))


def ell_abs_row_sums(num_rows, num_cols, width, pitch, Ax, row_sums, row_lengths=None, accumulate=False, stream=None):
    """row_sums[i] (+)= sum over the row's slots of |Ax[n * pitch + i]| (padding holds 0; the column indices are not read)."""
    import torch
    _need(Ax, "Ax", row_sums.dtype)
    _need(row_lengths, "row_lengths", torch.int32)
    _need(row_sums, "row_sums")
    if Ax.numel() < width * pitch or row_sums.numel() < num_rows:
        raise ValueError("ell_abs_row_sums: array lengths do not match the matrix shape")
    check(getattr(lib(), "cmi_ell_abs_row_sums_" + _suffix(row_sums))(num_rows, num_cols, width, pitch, None, _ptr(Ax), _ptr(row_lengths), _ptr(row_sums),
                                                                     int(bool(accumulate)), _stream(stream)))


def dia_abs_row_sums(num_rows, num_cols, num_diagonals, pitch, offsets, values, row_sums, accumulate=False, stream=None):
    """row_sums[i] (+)= sum of |values[d * pitch + i]| over the diagonals whose column i + offsets[d] lies inside the matrix."""
    import torch
    _need(offsets, "offsets", torch.int32)
    _need(values, "values", row_sums.dtype)
    _need(row_sums, "row_sums")
    if offsets.numel() != num_diagonals or values.numel() < num_diagonals * pitch or row_sums.numel() < num_rows:
        raise ValueError("dia_abs_row_sums: array lengths do not match the matrix shape")
    check(getattr(lib(), "cmi_dia_abs_row_sums_" + _suffix(row_sums))(num_rows, num_cols, num_diagonals, pitch, _ptr(offsets), _ptr(values), _ptr(row_sums),
                                                                     int(bool(accumulate)), _stream(stream)))


def random_fill(x, seed=0, stream=None):
    """x[i] <- uniform in [0, 1), a function of (i, seed) alone (cusp::random_array's values)."""
    _need(x, "x")
    check(getattr(lib(), "cmi_random_fill_" + _suffix(x))(x.numel(), int(seed), _ptr(x), _stream(stream)))


def blas_scal_recip(s, x, squared_norm=False, s_out=None, stream=None):
    """x <- (1 / s) x with s in device memory: 1 element of x's dtype, or (squared_norm) a float64 holding a norm's square.
    s_out (1 float64, optional) receives s."""
    import torch
    _need(s, "s", torch.float64 if squared_norm else x.dtype)
    _need(x, "x")
    _need(s_out, "s_out", torch.float64)
    check(getattr(lib(), "cmi_blas_scal_recip_" + _suffix(x))(x.numel(), _ptr(s), int(bool(squared_norm)), _ptr(x), _ptr(s_out), _stream(stream)))


class HostScalar:
    """8 bytes of page-locked, device-writable host memory (cmi_malloc_host) + the event that says a
    device value has landed in them: the CG convergence read without a blocking copy."""

    def __init__(self):
        L = lib()
        p, e = c_void_p(), c_void_p()
        check(L.cmi_malloc_host(byref(p), 8))
        self.ptr = p.value
        try:
            check(L.cmi_event_create(byref(e)))
        except Exception:
            L.cmi_free_host(self.ptr)
            self.ptr = None
            raise
        self.event = e.value

    def fetch(self, t, stream=None):
        """Queue device scalar -> host on the stream; returns at once."""
        check(lib().cmi_memcpy_d2h_async(self.ptr, _ptr(t), 8, _stream(stream)))
        self.record(stream)

    def record(self, stream=None):
        check(lib().cmi_event_record(self.event, _stream(stream)))

    def wait(self):
        check(lib().cmi_event_synchronize(self.event))
        return ctypes.c_double.from_address(self.ptr).value

    def close(self):
        if getattr(self, "ptr", None):
            L = lib()
            L.cmi_event_destroy(self.event)
            L.cmi_free_host(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


IPC_HANDLE_BYTES = 64
MAX_COPY_RANGES = 16


class DeviceBuffer:
    """An HBM allocation of its own (cmi_malloc, not a slice of torch's caching allocator), so that
    its IPC handle maps exactly this buffer in a peer process.  `tensor()` views it as a torch tensor."""

    def __init__(self, nbytes, device=None):
        import torch
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.nbytes = int(nbytes)
        p = c_void_p()
        with torch.cuda.device(self.device):
            check(lib().cmi_malloc(byref(p), max(self.nbytes, 8)))
            self.ptr = p.value
            check(lib().cmi_memset(self.ptr, 0, max(self.nbytes, 8), _stream(None)))

    def tensor(self, dtype):
        import torch
        item = torch.empty(0, dtype=dtype).element_size()
        typestr = {torch.float64: "<f8", torch.float32: "<f4", torch.int32: "<i4", torch.int64: "<i8", torch.uint8: "|u1"}[dtype]
        holder = _ArrayInterface(self, (self.nbytes // item,), typestr)
        t = torch.as_tensor(holder, device=self.device)
        if t.data_ptr() != self.ptr:
            raise CmiError(2, "DeviceBuffer.tensor: torch copied the buffer instead of viewing it")
        t._cmi_buffer = self  # the view keeps the allocation alive
        return t

    def ipc_handle(self):
        h = ctypes.create_string_buffer(IPC_HANDLE_BYTES)
        check(lib().cmi_ipc_get_handle(self.ptr, h))
        return h.raw

    def close(self):
        if getattr(self, "ptr", None):
            lib().cmi_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ArrayInterface:
    def __init__(self, owner, shape, typestr):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (owner.ptr, False), "version": 2,
                                         "strides": None}


def device_can_access_peer(device, peer_device):
    flag = c_int()
    check(lib().cmi_device_can_access_peer(int(device), int(peer_device), byref(flag)))
    return bool(flag.value)


def ipc_open(handle):
    """Map a peer process's DeviceBuffer; returns the device address valid in THIS process."""
    p = c_void_p()
    check(lib().cmi_ipc_open_handle(ctypes.create_string_buffer(handle, IPC_HANDLE_BYTES), byref(p)))
    return p.value


def ipc_close(ptr):
    check(lib().cmi_ipc_close_handle(ptr))


COMM_ID_BYTES = 128
OP_SUM, OP_MAX, OP_MIN = 0, 1, 2


def comm_library_version():
    """ncclGetVersion of the RCCL the library binds at run time; raises when it cannot be bound (local call, not collective)."""
    v = c_int()
    check(lib().cmi_comm_library_version(byref(v)))
    return v.value


class Comm:
    """cmi_comm: the RCCL communicator behind the C-ABI (include/cusp_mi355x.h, csrc/comm.hip) -- what the sharded SpMV / CG use for
    their data path: all-gather of x (equal or unequal pieces), grouped send/recv halo exchange, all-reduce of CG's scalars.  Every
    call is enqueued on the given (default: torch's current) stream.  The 128-byte unique id comes from rank 0 and reaches the other
    ranks through `broadcast` (any out-of-band channel: a torch.distributed store here, a TCP socket in the C++ layer)."""

    def __init__(self, rank, world, broadcast=None):
        raw, err = None, None
        if rank == 0:
            ident = ctypes.create_string_buffer(COMM_ID_BYTES)
            try:
                check(lib().cmi_comm_unique_id(ident))
                raw = ident.raw
            except CmiError as e:  # (RCCL not loadable: the other ranks must hear about it, not wait for an id that never comes)
                err = e
        if world > 1:
            if broadcast is None:
                raise ValueError("Comm: a multi-rank communicator needs a broadcast function for the unique id")
            raw = broadcast(raw if rank == 0 else None)
        if raw is None:
            raise err if err is not None else CmiError(7, "CMI_ERROR_COMM: rank 0 could not make a communicator id")
        self._h = c_void_p()
        self.rank, self.world = rank, world
        check(lib().cmi_comm_create(ctypes.create_string_buffer(raw, COMM_ID_BYTES), rank, world, byref(self._h)))

    @classmethod
    def from_torch_distributed(cls, group=None):
        """One communicator per process group, made collectively: rank 0's id travels through torch.distributed's object broadcast
        (control plane only -- the data path is then this communicator's)."""
        import torch.distributed as dist
        key = id(group) if group is not None else 0
        if key not in _comms:
            rank, world = dist.get_rank(group), dist.get_world_size(group)

            def bcast(raw):
                box = [raw]
                dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
                return box[0]
            _comms[key] = cls(rank, world, bcast)
        return _comms[key]

    @property
    def handle(self):
        return self._h

    def library_version(self):
        return comm_library_version()

    def allgather(self, send, recv, count, stream=None):
        """recv[r*count, +count) <- rank r's send[0, count); in place when send is recv's own slice."""
        check(getattr(lib(), "cmi_allgather_" + _suffix(recv))(self._h, _ptr(send), _ptr(recv), int(count), _stream(stream)))

    def allgatherv(self, send, recv, counts, displs, algorithm=1, stream=None):
        c = (c_int64 * self.world)(*[int(v) for v in counts])
        d = (c_int64 * self.world)(*[int(v) for v in displs])
        check(getattr(lib(), "cmi_allgatherv_" + _suffix(recv))(self._h, _ptr(send), _ptr(recv), c, d, int(algorithm), _stream(stream)))

    def halo_exchange(self, x_full, peers, send_lo, send_n, recv_lo, recv_n, stream=None):
        n = len(peers)
        arr = lambda v: (c_int64 * max(n, 1))(*[int(t) for t in v])  # noqa: E731
        check(getattr(lib(), "cmi_halo_exchange_" + _suffix(x_full))(self._h, _ptr(x_full), n, (c_int * max(n, 1))(*peers), arr(send_lo), arr(send_n),
                                                                     arr(recv_lo), arr(recv_n), _stream(stream)))

    def allreduce(self, t, op=OP_SUM, stream=None):
        """in-place all-reduce of a float64 device tensor (CG's scalars)"""
        import torch
        if t.dtype != torch.float64:
            raise TypeError("Comm.allreduce: float64 tensors only")
        check(lib().cmi_allreduce_f64(self._h, _ptr(t), _ptr(t), t.numel(), int(op), _stream(stream)))

    def barrier(self, stream=None):
        check(lib().cmi_comm_barrier(self._h, _stream(stream)))

    def allgather_host(self, record):
        """bytes -> list of every rank's bytes (small set-up records)"""
        out = ctypes.create_string_buffer(len(record) * self.world)
        check(lib().cmi_comm_allgather_host(self._h, record, out, len(record), _stream(None)))
        return [out.raw[i * len(record):(i + 1) * len(record)] for i in range(self.world)]

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.cmi_comm_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


_comms = {}


def csr_column_span(Aj, stream=None):
    """(smallest, largest) column index on the device; (0, -1) for no entries."""
    lo, hi = ctypes.c_int32(), ctypes.c_int32()
    check(lib().cmi_csr_column_span(Aj.numel(), _ptr(Aj), byref(lo), byref(hi), _stream(stream)))
    return lo.value, hi.value


class CopyRanges:
    """A fixed list of (src address, dst address, bytes) copied by ONE launch (cmi_copy_ranges)."""

    def __init__(self, ranges):
        ranges = [r for r in ranges if r[2] > 0]
        if len(ranges) > MAX_COPY_RANGES:
            raise ValueError(f"at most {MAX_COPY_RANGES} ranges per launch")
        n = len(ranges)
        self.n = n
        self.src = (c_void_p * max(n, 1))(*[r[0] for r in ranges])
        self.dst = (c_void_p * max(n, 1))(*[r[1] for r in ranges])
        self.bytes = (c_int64 * max(n, 1))(*[r[2] for r in ranges])

    def launch(self, stream=None):
        if self.n:
            check(lib().cmi_copy_ranges(self.n, self.src, self.dst, self.bytes, _stream(stream)))


def cg_direction(rr_new, rr_old, r, p, stream=None):
    """beta = rr_new/rr_old (device scalars); p = r + beta p."""
    check(getattr(lib(), "cmi_cg_direction_" + _suffix(p))(p.numel(), _ptr(rr_new), _ptr(rr_old), _ptr(r), _ptr(p), _stream(stream)))


def cg_direction_x(rr_new, rr_old, yp, r, p, x, stream=None):
    """alpha = rr_old/yp, beta = rr_new/rr_old (device scalars); x += alpha p (old p), then p = r + beta p -- one pass."""
    check(getattr(lib(), "cmi_cg_direction_x_" + _suffix(p))(p.numel(), _ptr(rr_new), _ptr(rr_old), _ptr(yp), _ptr(r), _ptr(p), _ptr(x),
                                                             _stream(stream)))


def blas_dotd(x, y, result, workspace, stream=None):
    """<x, y> as a DOUBLE in device memory whatever the vectors' type (the scalar type of the fused CG steps)."""
    import torch
    if x.dtype == torch.float64:
        check(lib().cmi_blas_dot_f64(x.numel(), _ptr(x), _ptr(y), _ptr(result), _ptr(workspace), _stream(stream)))
    else:
        check(lib().cmi_blas_dotd_f32(x.numel(), _ptr(x), _ptr(y), _ptr(result), _ptr(workspace), _stream(stream)))


def coo_row_offsets(num_rows, Ai, Ap, stream=None):
    """Ap[num_rows + 1] <- row offsets of row-sorted COO row indices (device); returns False (Ap unspecified) when the
    entries turn out not to be sorted by row."""
    import torch
    _need(Ai, "Ai", torch.int32)
    _need(Ap, "Ap", torch.int32)
    ok = ctypes.c_int(0)
    check(lib().cmi_coo_row_offsets(num_rows, Ai.numel(), _ptr(Ai), _ptr(Ap), byref(ok), _stream(stream)))
    return bool(ok.value)


def csr_interior_rows(num_rows, Ap, Aj, col_lo, col_hi, stream=None):
    """(first, last): rows [first, last) of a row block reference only columns in [col_lo, col_hi) -- the rows a sharded multiply can run
    while the halo is in flight (cmi_csr_interior_rows)."""
    import torch
    _need(Ap, "Ap", torch.int32)
    _need(Aj, "Aj", torch.int32)
    a, b = c_int64(0), c_int64(0)
    check(lib().cmi_csr_interior_rows(num_rows, _ptr(Ap), _ptr(Aj), col_lo, col_hi, byref(a), byref(b), _stream(stream)))
    return a.value, b.value


def coo_sort_by_row(num_rows, num_cols, Ai, Aj, Ax, and_column=False, stream=None):
    """In-place STABLE sort of COO entries by row (and_column: by (row, column)) on the device -- coo_matrix::sort_by_row
    (cusp/coo_matrix.h:208-212, cusp/sort.h:231,302).  Entries of one row keep their storage order."""
    import torch
    _need(Ai, "Ai", torch.int32)
    _need(Aj, "Aj", torch.int32)
    if not (Ai.numel() == Aj.numel() == Ax.numel()):
        raise ValueError("coo_sort_by_row: the three arrays differ in length")
    fn = getattr(lib(), "cmi_coo_sort_by_row_" + _suffix(Ax))
    check(fn(num_rows, num_cols, Ai.numel(), _ptr(Ai), _ptr(Aj), _ptr(Ax), 1 if and_column else 0, _stream(stream)))


def coo_is_sorted(num_rows, Ai, Aj=None, and_column=False, stream=None):
    """is_sorted_by_row / is_sorted_by_row_and_column (cusp/coo_matrix.h:218-224) on the device."""
    import torch
    _need(Ai, "Ai", torch.int32)
    if and_column:
        _need(Aj, "Aj", torch.int32)
    ok = ctypes.c_int(0)
    check(lib().cmi_coo_is_sorted(num_rows, Ai.numel(), _ptr(Ai), _ptr(Aj) if Aj is not None else None, 1 if and_column else 0, byref(ok), _stream(stream)))
    return bool(ok.value)


def ell_to_csr(num_rows, width, pitch, ell_Aj, ell_Ax, stream=None):
    """(Ap, Aj, Ax) of the entries of an ELL matrix with a valid column, row by row, built on the device."""
    import torch
    fn = getattr(lib(), "cmi_ell_to_csr_" + _suffix(ell_Ax))
    dev = ell_Ax.device
    Ap = torch.empty(num_rows + 1, dtype=torch.int32, device=dev)
    n = c_int64(0)
    check(fn(num_rows, width, pitch, _ptr(ell_Aj), _ptr(ell_Ax), _ptr(Ap), None, None, 0, byref(n), _stream(stream)))
    Aj = torch.empty(n.value, dtype=torch.int32, device=dev)
    Ax = torch.empty(n.value, dtype=ell_Ax.dtype, device=dev)
    if n.value:
        check(fn(num_rows, width, pitch, _ptr(ell_Aj), _ptr(ell_Ax), _ptr(Ap), _ptr(Aj), _ptr(Ax), n.value, byref(n), _stream(stream)))
    return Ap, Aj, Ax


def dia_to_csr(num_rows, num_cols, num_diagonals, pitch, offsets, values, stream=None):
    """(Ap, Aj, Ax) of the non-zero entries of a DIA matrix with a valid column, row by row, built on the device."""
    import torch
    fn = getattr(lib(), "cmi_dia_to_csr_" + _suffix(values))
    dev = values.device
    Ap = torch.empty(num_rows + 1, dtype=torch.int32, device=dev)
    n = c_int64(0)
    check(fn(num_rows, num_cols, num_diagonals, pitch, _ptr(offsets), _ptr(values), _ptr(Ap), None, None, 0, byref(n), _stream(stream)))
    Aj = torch.empty(n.value, dtype=torch.int32, device=dev)
    Ax = torch.empty(n.value, dtype=values.dtype, device=dev)
    if n.value:
        check(fn(num_rows, num_cols, num_diagonals, pitch, _ptr(offsets), _ptr(values), _ptr(Ap), _ptr(Aj), _ptr(Ax), n.value, byref(n),
                 _stream(stream)))
    return Ap, Aj, Ax


def hyb_to_csr(num_rows, width, pitch, ell_Aj, ell_Ax, coo_Ai, coo_Aj, coo_Ax, stream=None):
    """(Ap, Aj, Ax): each row's ELL entries, then its COO entries (row-sorted COO part), built on the device."""
    import torch
    fn = getattr(lib(), "cmi_hyb_to_csr_" + _suffix(ell_Ax))
    dev = ell_Ax.device
    Ap = torch.empty(num_rows + 1, dtype=torch.int32, device=dev)
    n = c_int64(0)
    args = (num_rows, width, pitch, _ptr(ell_Aj), _ptr(ell_Ax), coo_Ai.numel(), _ptr(coo_Ai), _ptr(coo_Aj), _ptr(coo_Ax), _ptr(Ap))
    check(fn(*args, None, None, 0, byref(n), _stream(stream)))
    Aj = torch.empty(n.value, dtype=torch.int32, device=dev)
    Ax = torch.empty(n.value, dtype=ell_Ax.dtype, device=dev)
    if n.value:
        check(fn(*args, _ptr(Aj), _ptr(Ax), n.value, byref(n), _stream(stream)))
    return Ap, Aj, Ax
