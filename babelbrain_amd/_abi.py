"""The C ABI of libbabelfdtd_hip.so as data: one signature per entry of include/babelfdtd.h, the two structs, and the loader
that applies them. tests/test_abi_cpu.py holds every line here to the header's prototypes; no library is needed for that."""
import ctypes as C
import os

ABI_VERSION = 7         # BFD_ABI_VERSION of the header

# BABELFDTD_HIP_LIB: another build of the same library (A/B kernel experiments, scripts/ab_build.sh)
LIB_PATH = os.environ.get('BABELFDTD_HIP_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libbabelfdtd_hip.so')


class EngineError(RuntimeError):
    pass


class Config(C.Structure):
    """bfd_config of include/babelfdtd.h"""
    _fields_ = [('N1', C.c_int32), ('N2', C.c_int32), ('N3', C.c_int32), ('k0', C.c_int32), ('nk', C.c_int32),
                ('nMat', C.c_int32), ('NDelta', C.c_int32), ('typeSource', C.c_int32), ('sensorSub', C.c_int32),
                ('sensorStart', C.c_int32), ('nt', C.c_int32), ('selRMSorPeak', C.c_int32),
                ('selMapsRMS', C.c_uint32), ('selMapsSensors', C.c_uint32), ('qfactorCorrection', C.c_int32),
                ('device', C.c_int32), ('kernelVariant', C.c_int32), ('rmsFirstStep', C.c_int32), ('sensorMode', C.c_int32),
                ('h', C.c_double), ('dt', C.c_double), ('freq', C.c_double), ('reflectionLimit', C.c_double)]


class PackSpec(C.Structure):
    """bfd_pack_spec of include/babelfdtd.h"""
    _fields_ = [('lo', C.c_int32 * 3), ('hi', C.c_int32 * 3), ('zSource', C.c_int32), ('O', C.c_int32 * 3), ('at', C.c_int32 * 3),
                ('flipK', C.c_int32), ('applyScale', C.c_int32), ('ampScale', C.c_double), ('correction', C.c_double)]


# Argument types. ptr: a handle or an array the caller passes as an address (_ptr, a raw stream or device address, None);
# p_*: one value passed with byref. `int` and `int32_t` of the header are both i32.
ptr, cstr, i32, u32, i64, f32, f64 = C.c_void_p, C.c_char_p, C.c_int32, C.c_uint32, C.c_int64, C.c_float, C.c_double
p_ptr, p_i32, p_u32, p_i64, p_size, p_f32, p_f64 = (C.POINTER(t) for t in (ptr, i32, u32, i64, C.c_size_t, f32, f64))
p_config, p_pack = C.POINTER(Config), C.POINTER(PackSpec)

# Runs of arguments that several entries share
STRIDES = [i64, i64, i64]                                   # s1, s2, s3: element strides of a volume
SOURCES = [ptr, i64, ptr, ptr, ptr, ptr, ptr]               # handle, nVox, index, row, wx, wy, wz
SOURCES_DENSE = SOURCES + [ptr, i32, i32]                   # + pulse, nSources, nT
SOURCES_SEPARABLE = SOURCES + [i32, i32, ptr, i32, ptr]     # + nSources, K, weights, nT, signals
BHTE_VOLUMES = [i32, i32, i32, i32, i32, ptr, ptr, ptr, ptr, ptr, i32, ptr, ptr, ptr, ptr, i32, f32, f64, i32, ptr,
                i32, i32, ptr, i64, ptr, ptr, p_f64]        # bfd_bhte_run_volumes; the material map is uint16 in the ...16 entries
BHTE_PROTOCOL = BHTE_VOLUMES + [i32, ptr, ptr, ptr]         # + nCaptures, captureStep, Tmax, doseAtCapture

# entry -> (restype, argtypes), in the header's order
SIGNATURES = {
    'bfd_abi_version': (i32, []),
    'bfd_last_error': (cstr, []),
    'bfd_device_count': (i32, []),
    'bfd_device_name': (i32, [i32, cstr, i32]),
    'bfd_stable_dt': (f64, [i32, ptr, ptr, f64, i32, f64, f64]),
    'bfd_material_tables': (i32, [i32, ptr, ptr, f64, i32, f64, f64, ptr, ptr, ptr]),
    # one engine
    'bfd_create': (i32, [p_config, p_ptr]),
    'bfd_destroy': (None, [ptr]),
    'bfd_set_stream': (i32, [ptr, ptr]),
    'bfd_use_private_stream': (i32, [ptr]),
    'bfd_set_materials': (i32, [ptr, ptr, ptr]),
    'bfd_set_material_map': (i32, [ptr, ptr] + STRIDES + [i32, i32]),
    'bfd_set_reflector': (i32, [ptr, ptr] + STRIDES),
    'bfd_set_sources': (i32, SOURCES_DENSE),
    'bfd_set_sources_separable': (i32, SOURCES_SEPARABLE),
    'bfd_set_sensor_map': (i32, [ptr, ptr] + STRIDES + [p_i64]),
    'bfd_set_material_map_device': (i32, [ptr, ptr] + STRIDES + [i32, i32]),
    'bfd_set_reflector_device': (i32, [ptr, ptr] + STRIDES),
    'bfd_set_sensor_box': (i32, [ptr, ptr, ptr, p_i64]),
    'bfd_run': (i32, [ptr, i32]),
    'bfd_half_step_stress': (i32, [ptr]),
    'bfd_half_step_velocity': (i32, [ptr]),
    'bfd_half_step_stress_part': (i32, [ptr, i32]),
    'bfd_half_step_velocity_part': (i32, [ptr, i32]),
    'bfd_half_step_stress_part_on': (i32, [ptr, i32, ptr]),
    'bfd_half_step_velocity_part_on': (i32, [ptr, i32, ptr]),
    'bfd_sync': (i32, [ptr]),
    'bfd_current_step': (i32, [ptr]),
    'bfd_prepare': (i32, [ptr]),
    'bfd_placement_note': (cstr, [ptr]),
    'bfd_set_placement': (i32, [ptr, i32, i64]),
    'bfd_placement_cache_release': (i64, []),
    'bfd_halo_region': (i32, [ptr, i32, i32, i32, i32, p_ptr, p_size]),
    'bfd_halo_fields': (i32, [ptr, i32, p_u32]),
    'bfd_timing_begin': (i32, [ptr, i32]),
    'bfd_timing_end': (i32, [ptr, p_f64, p_f64, p_f64, p_f64, p_i64, p_i64]),
    'bfd_timing_kernels': (i32, [ptr, ptr, ptr]),
    'bfd_algorithmic_bytes': (i32, [ptr, i32, ptr]),
    'bfd_paired_launches': (i64, [ptr]),
    'bfd_reset': (i32, [ptr]),
    'bfd_num_sensors': (i64, [ptr]),
    'bfd_num_sensor_steps': (i32, [ptr]),
    'bfd_get_sensor_index': (i32, [ptr, ptr]),
    'bfd_get_sensors': (i32, [ptr, ptr]),
    'bfd_get_sensor_dft': (i32, [ptr, f64, ptr, ptr]),
    'bfd_dft_series': (i32, [i32, i64, i32, ptr, f64, f64, ptr, ptr]),
    'bfd_pack_results': (i32, [ptr, p_pack, ptr, ptr, ptr, p_f32]),
    'bfd_get_map': (i32, [ptr, i32, i32, ptr] + STRIDES),
    'bfd_get_field': (i32, [ptr, i32, ptr] + STRIDES),
    'bfd_tile_counts': (i32, [ptr, p_i32, p_i32, p_i32, p_i32, p_i32]),
    'bfd_tile_count_lean': (i32, [ptr, p_i32]),
    'bfd_tile_count_fused': (i32, [ptr, p_i32]),
    'bfd_activity_counts': (i32, [ptr, p_i64, p_i64]),
    'bfd_device_bytes': (i64, [ptr]),
    # a group of engines
    'bfd_group_create': (i32, [p_config, i32, ptr, p_ptr]),
    'bfd_group_destroy': (None, [ptr]),
    'bfd_group_size': (i32, [ptr]),
    'bfd_group_slab': (i32, [ptr, i32, p_i32, p_i32, p_i32, p_ptr]),
    'bfd_group_set_materials': (i32, [ptr, ptr, ptr]),
    'bfd_group_set_material_map': (i32, [ptr, ptr] + STRIDES),
    'bfd_group_set_reflector': (i32, [ptr, ptr] + STRIDES),
    'bfd_group_set_sources': (i32, SOURCES_DENSE),
    'bfd_group_set_sources_separable': (i32, SOURCES_SEPARABLE),
    'bfd_group_set_sensor_map': (i32, [ptr, ptr] + STRIDES + [p_i64]),
    'bfd_group_set_placement': (i32, [ptr, i32, i64]),
    'bfd_group_prepare': (i32, [ptr]),
    'bfd_group_run': (i32, [ptr, i32]),
    'bfd_group_sync': (i32, [ptr]),
    'bfd_group_reset': (i32, [ptr]),
    'bfd_group_timing_begin': (i32, [ptr]),
    'bfd_group_timing_end': (i32, [ptr, p_f64, p_f64, p_f64, p_f64, p_i32]),
    'bfd_group_peer_status': (i32, [ptr, ptr, i32]),
    'bfd_group_num_sensors': (i64, [ptr]),
    'bfd_group_num_sensor_steps': (i32, [ptr]),
    'bfd_group_get_sensor_index': (i32, [ptr, ptr]),
    'bfd_group_get_sensors': (i32, [ptr, ptr]),
    'bfd_group_get_sensor_dft': (i32, [ptr, f64, ptr, ptr]),
    'bfd_group_get_map': (i32, [ptr, i32, i32, ptr] + STRIDES),
    'bfd_group_device_bytes': (i64, [ptr]),
    # Rayleigh integral and bio-heat
    'bfd_rayleigh_forward': (i32, [i32, i64, ptr, ptr, ptr, f64, f64, i64, ptr, ptr, p_f64]),
    'bfd_rayleigh_forward_elements': (i32, [i32, i64, ptr, ptr, ptr, i32, ptr, i32, ptr, f64, f64, i64, ptr, ptr, p_f64]),
    'bfd_bhte_run': (i32, [i32, i32, i32, i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, f32, f64, i32, i32, i32, i32, ptr, i64, ptr, ptr, p_f64]),
    'bfd_bhte_run_fields': (i32, [i32, i32, i32, i32, i32, ptr, ptr, ptr, i32, ptr, ptr, ptr, f32, f64, i32, ptr, i32, i32, ptr, i64, ptr, ptr, p_f64]),
    'bfd_bhte_run_volumes': (i32, BHTE_VOLUMES),
    'bfd_bhte_run_protocol': (i32, BHTE_PROTOCOL),
    'bfd_bhte_max_materials': (i32, []),
    'bfd_bhte_run_volumes16': (i32, BHTE_VOLUMES),
    'bfd_bhte_run_protocol16': (i32, BHTE_PROTOCOL),
    # Step-1, domain and analysis calls on whole volumes
    'bfd_median_filter3d': (i32, [i32, i32, ptr, ptr, ptr, i64, i64, i64, i32, i32, i32, i32, f64, p_f32]),
    'bfd_binary_morphology3d': (i32, [i32, i32, ptr, ptr, i64, i64, i64, ptr, i32, i32, i32, i32, i32, p_f32]),
    'bfd_label3d': (i32, [i32, ptr, ptr, i64, i64, i64, i32, p_i64, ptr, i64, ptr, p_f32]),
    'bfd_affine_transform3d': (i32, [i32, i32, ptr, ptr, i64, i64, i64, i64, i64, i64, ptr, i32, i32, f64, i32, ptr]),
    'bfd_spline_filter3d': (i32, [i32, i32, ptr, ptr, i64, i64, i64, i32, i32, p_f32]),
    'bfd_voxelize_mesh': (i32, [i32, ptr, i64, ptr, ptr, i64, i64, i64, ptr, ptr, p_i64, p_f32]),
    'bfd_voxel_points': (i32, [i32, ptr, i64, i64, i64, ptr, ptr, ptr, i64, p_i64, p_f32]),
    'bfd_voxel_scatter3d': (i32, [i32, ptr, i64, i64, i64, ptr, ptr, ptr, i64, i64, i64, ptr, ptr, ptr, ptr, p_f32]),
    'bfd_voxelize_scatter3d': (i32, [i32, ptr, i64, ptr, ptr, i64, i64, i64, ptr, i64, i64, i64, ptr, ptr, ptr, ptr, p_f32]),
    'bfd_map_values3d': (i32, [i32, ptr, ptr, ptr, i64, ptr, i64, p_f32]),
    'bfd_distance_transform_edt3d': (i32, [i32, ptr, i32, ptr, ptr, i64, i64, i64, p_f32]),
    'bfd_gaussian_filter3d': (i32, [i32, i32, ptr, ptr, i64, i64, i64, p_f64, f64, i32, f64, p_f32]),
    'bfd_paint_components3d': (i32, [i32, ptr, ptr, i64, i64, i64, i32, i32, i32, i32, ptr, p_f32]),
    'bfd_quantize_values3d': (i32, [i32, ptr, ptr, i64, i64, i64, i32, ptr, ptr, ptr, p_i64, ptr, p_f32]),
    'bfd_clear_beyond_bone3d': (i32, [i32, ptr, ptr, i64, i64, i64, i64, i32, i32, i32, i32, ptr, p_f32]),
    'bfd_label_survey3d': (i32, [i32, ptr, i64, i64, i64, ptr, ptr, i32, ptr, ptr, ptr, p_f32]),
    'bfd_assemble_material_map3d': (i32, [i32, ptr, ptr, i32, ptr, i64, i64, i64, ptr, ptr, ptr, ptr, i32, ptr, u32, i64, i64, ptr, ptr, ptr, ptr, ptr,
                                          p_f32]),
    'bfd_sdr_rays3d': (i32, [i32, ptr, i32, i64, i64, i64, ptr, ptr, i32, ptr, i32, i64, i64, i64, i64, f64, ptr, ptr, ptr, p_f32]),
    'bfd_integer_histogram3d': (i32, [i32, i32, ptr, i64, i64, i64, ptr, p_i64, p_i64, ptr, p_f32]),
    'bfd_order_statistics3d': (i32, [i32, i32, ptr, ptr, i64, i64, i64, f64, i32, ptr, i32, f64, p_i64, ptr, ptr, p_f32]),
    'bfd_uniform_histogram3d': (i32, [i32, i32, ptr, i64, i64, i64, f64, i32, i32, ptr, ptr, ptr, p_i64, p_f32]),
    'bfd_pseudo_ct_candidates3d': (i32, [i32, i32, ptr, i64, i64, i64, f64, ptr, ptr, f64, f64, ptr, p_f64, p_i64, p_f32]),
    'bfd_pseudo_ct_convert3d': (i32, [i32, i32, ptr, i64, i64, i64, f64, ptr, ptr, ptr, ptr, f64, f64, i32, ptr, p_f32]),
    'bfd_select_component3d': (i32, [i32, ptr, ptr, i64, i64, i64, i32, i32, ptr, p_f32]),
    'bfd_bone_rim_correct3d': (i32, [i32, ptr, ptr, ptr, i64, i64, i64, ptr, f32, f64, f64, f64, ptr, ptr, i32, ptr, ptr, ptr, ptr, ptr, p_f32]),
    'bfd_class_extrema3d': (i32, [i32, ptr, i32, ptr, i32, i64, i64, i64, ptr, i32, ptr, ptr, ptr, ptr, ptr, p_f32]),
    'bfd_loss_survey3d': (i32, [i32, ptr, ptr, i32, ptr, i32, i64, i64, i64, ptr, i32, ptr, ptr, ptr, f64, f64, f64, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr,
                                p_f32]),
    # the thermal study
    'bfd_thermal_create': (i32, [i32, i64, i64, i64, i32, i32, p_ptr]),
    'bfd_thermal_destroy': (None, [ptr]),
    'bfd_thermal_set_inputs': (i32, [ptr, ptr, ptr, ptr, i32]),
    'bfd_thermal_median_region': (i32, [ptr, ptr, i32, i32, p_f32]),
    'bfd_thermal_loss_survey': (i32, [ptr, ptr, ptr, ptr, ptr, f64, f64, f64, ptr, ptr, ptr, ptr, ptr, ptr, ptr, p_f32]),
    'bfd_thermal_set_scale': (i32, [ptr, ptr, i32]),
    'bfd_thermal_run': (i32, [ptr, ptr, ptr, ptr, ptr, i32, ptr, ptr, f32, f64, i32, ptr, i32, i64, ptr, ptr, i32, ptr, p_f64]),
    'bfd_thermal_set_previous': (i32, [ptr, ptr, ptr, ptr]),
    'bfd_thermal_merge_max': (i32, [ptr, i32, ptr]),
    'bfd_thermal_extrema': (i32, [ptr, ptr, i32, ptr, ptr, ptr, ptr, ptr, ptr, p_f32]),
    'bfd_thermal_get': (i32, [ptr, i32, ptr, i32]),
    'bfd_thermal_get_plane': (i32, [ptr, i32, i64, ptr]),
    'bfd_thermal_traffic': (i32, [ptr, p_i64, p_i64]),
    # the acoustic study
    'bfd_acoustic_create': (i32, [i32, i64, i64, i64, i32, i32, p_ptr]),
    'bfd_acoustic_destroy': (None, [ptr]),
    'bfd_acoustic_set_volumes': (i32, [ptr, ptr, ptr, ptr]),
    'bfd_acoustic_survey': (i32, [ptr, ptr, ptr, i32, ptr, ptr, ptr]),
    'bfd_acoustic_assemble': (i32, [ptr, ptr, ptr, ptr, ptr, i32, ptr, u32, i64, i64, ptr, i32, ptr]),
    'bfd_acoustic_attach': (i32, [ptr, ptr]),
    'bfd_acoustic_pack': (i32, [ptr, ptr, p_pack, i32]),
    'bfd_acoustic_get': (i32, [ptr, i32, i32, ptr]),
    'bfd_acoustic_traffic': (i32, [ptr, p_i64, p_i64]),
}
ABI_SYMBOLS = list(SIGNATURES)      # every symbol include/babelfdtd.h declares (tests check that the library exports all of them)
OPTIONAL = {'bfd_paired_launches'}  # absent in older builds selected with BABELFDTD_HIP_LIB


def _preload_torch_hip_runtime():
    """One HIP runtime per process. PyTorch-ROCm wheels bundle their own libamdhip64 (soname
    libamdhip64.so.7, the one this library needs too). If this library were loaded first it would bind to
    the system runtime and a later `import torch` would bring a second one, which then finds no GPU. So when
    a torch wheel is installed its runtime is loaded first (a plain dlopen, torch itself is not imported);
    multi-GPU runs (slab.py) hand torch streams and RCCL the engine's device memory and need the shared runtime."""
    import importlib.util
    import sys
    if 'torch' in sys.modules:
        return
    try:
        spec = importlib.util.find_spec('torch')
    except Exception:
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], 'lib', 'libamdhip64.so')
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library(path):
    """Load the library at `path` and give every entry its signature; raises if it has not been built (python __graft_entry__.py build)."""
    if not os.path.exists(path):
        raise EngineError('HIP engine library missing: %s (build it with `make -C babelbrain_amd/csrc`); '
                          'there is no CPU fallback' % path)
    _preload_torch_hip_runtime()
    lib = C.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        if name in OPTIONAL and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.bfd_abi_version() != ABI_VERSION:
        raise EngineError('libbabelfdtd_hip.so ABI version mismatch')
    return lib
