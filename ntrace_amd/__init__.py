"""ntrace_amd -- MI355X-native tracer backend for NTrace (BVH trace + LBVH / HLBVH / binned SAH builds, kd-tree build (host and device) + trace).

The product is libntrace_amd.so (hand-written HIP kernels for gfx950 behind the C-ABI
of include/ntrace_amd.h) plus the C++ host mirror of the reference's Renderer / CudaBVH /
RayBuffer classes in ntrace_amd/host.  This Python module is plumbing for tests and
bench.py: it loads the library with ctypes and passes raw device pointers (e.g. torch
tensors' data_ptr()).  There is no CPU or PyTorch fallback: if the library is missing the
import of `ntrace_amd.lib()` fails loudly.
"""
from ._capi import (BvhView, RAY_DTYPE, RESULT_DTYPE, HostBvh, KernelConfig, NtrError, TraceStats, bvh_validate, lib,
                    lib_path, query_config, sah_build, trace_bvh, trace_bvh_stats, pixel_table,
                    raygen_primary, raygen_ao, raygen_shadow, count_hits, selftest_division, selftest_division_hard, selftest_ray_class, bvh_leaf_depths, secondary_block_costs, lbvh_capacity,
                    lbvh_build, LbvhResult, hlbvh_build, HlbvhResult, reconstruct, ray_morton_sort, camera_decode, camera_reencode,
                    camera_nscreen_to_world, obj_load, SchedHint, trace_status, trace_plan, trace_plan_hint_step, trace_plan_certain, TracePlan, set_tunables, host_bvh_wrap, use_library, trace_graph_reserve, trace_graph_release_all, stream_release, selftest_auto_hint_table, selftest_gather_rate, frame_shard, frame_ao_batches, DistGroup,
                    lbvh_release_workspace, predict_block_costs, predict_batch_coherence, predict_dispatch_order, SchedHintState,
                    HostKdtree, kdtree_build, host_kdtree_wrap, trace_kdtree, KDTREE_SPATIAL_MEDIAN, KDTREE_SAH,
                    DeviceKdtree, KdtreeDeviceParams, kdtree_device_build, kdtree_device_params, KDTREE_DEVICE_DEFAULTS,
                    kdtree_device_scratch_bytes, PersistentBvhParams, PersistentBvhResult, persistent_bvh_params,
                    persistent_bvh_build, persistent_bvh_scratch_bytes, PERSISTENT_BVH_DEFAULTS, SahDeviceResult,
                    sah_device_build, sah_device_scratch_bytes, BvhRefitResult, bvh_refit,
                    bvh_refit_scratch_bytes, BvhOptimizeResult, BvhSahResult, bvh_optimize, bvh_optimize_scratch_bytes, bvh_sah_cost,
                    BvhReorderResult, bvh_reorder, bvh_reorder_scratch_bytes,
                    PlocResult, ploc_build, ploc_scratch_bytes, PLOC_TAIL, PLOC_TILE,
                    PlocBatchMesh, PlocBatchMeshResult, PlocBatchResult, ploc_batch_capacity, ploc_build_batch, ploc_batch_scratch_bytes,
                    RefitBatchEntry, BvhRefitBatchResult, bvh_refit_batch, bvh_refit_batch_scratch_bytes,
                    INSTANCE_DTYPE, BlasRange, BlasPool, TlasResult, instance_invert, make_instances, tlas_capacity, tlas_build,
                    tlas_scratch_bytes, trace_instanced, InstanceVisibility, InstancedTraceStats,
                    trace_instanced_masked, trace_instanced_stats, TlasRefitResult, tlas_refit, tlas_refit_scratch_bytes,
                    BlasTris, BLAS_TRIS_DTYPE, InstancedGeometry, instanced_hit_attributes, raygen_ao_normals,
                    BvhWideResult, bvh_widen_capacity, bvh_widen, bvh_widen_scratch_bytes, trace_wide, trace_wide_stats,
                    WideBlasRange, TlasWideResult, InstancedWideTraceStats, pool_widen_capacity, pool_widen, tlas_widen,
                    pool_widen_batch, pool_widen_batch_scratch_bytes,
                    BvhOptimizeBatchEntry, BvhOptimizeBatchResult, BvhSahBatchResult, bvh_optimize_batch, bvh_optimize_batch_scratch_bytes,
                    bvh_sah_cost_batch, OPT_ERR_LINK, OPT_ERR_ROW, OPT_ERR_NO_TREE,
                    trace_instanced_wide, trace_instanced_wide_stats,
                    instanced_validate, instanced_flags_read, trace_instanced_fast, trace_instanced_fast_stats, InstancedFastStats,
                    instanced_wide_validate, trace_instanced_wide_fast, trace_instanced_wide_fast_stats,
                    trace_instanced_seeded, trace_instanced_seeded_stats, trace_instanced_wide_seeded, trace_instanced_wide_seeded_stats,
                    WideRefitEntry, WideRefitResult, pool_wide_refit, pool_wide_refit_scratch_bytes, tlas_wide_refit,
                    tlas_wide_refit_scratch_bytes,
                    InstancesUpdateResult, instances_update, instances_status_read, instances_update_host, INSTANCE_MAX_CHAIN,
                    INSTANCE_ERR_SINGULAR, INSTANCE_ERR_CHAIN,
                    TlasMotionRefitResult, InstanceMotion, InstancedMotionStats, tlas_motion_refit, tlas_motion_refit_scratch_bytes,
                    trace_instanced_motion, trace_instanced_motion_stats, instanced_hit_attributes_motion, ray_times_primary,
                    ray_times_secondary)

BVHLayout_Compact = 4
BVH_FINITE, BVH_FASTDIV, BVH_NOTINY, BVH_ORDERED, BVH_WIDE_LEAVES = 1, 2, 4, 8, 16
KERNELS = ("fermi_speculative_while_while", "tesla_persistent_while_while",
           "tesla_persistent_speculative_while_while", "kepler_dynamic_fetch")

__all__ = ["BvhView", "RAY_DTYPE", "RESULT_DTYPE", "HostBvh", "KernelConfig", "NtrError", "bvh_validate", "lib",
           "lib_path", "query_config", "sah_build", "trace_bvh", "trace_bvh_stats", "TraceStats", "pixel_table", "raygen_primary", "raygen_ao", "count_hits", "selftest_division", "selftest_division_hard", "selftest_ray_class", "bvh_leaf_depths", "secondary_block_costs", "lbvh_capacity", "lbvh_build", "LbvhResult", "hlbvh_build", "HlbvhResult", "reconstruct", "ray_morton_sort", "camera_decode", "camera_reencode", "camera_nscreen_to_world", "obj_load", "SchedHint", "trace_status", "set_tunables", "host_bvh_wrap", "BVHLayout_Compact", "KERNELS",
           "HostKdtree", "kdtree_build", "host_kdtree_wrap", "trace_kdtree", "KDTREE_SPATIAL_MEDIAN", "KDTREE_SAH",
           "DeviceKdtree", "KdtreeDeviceParams", "kdtree_device_build", "kdtree_device_params", "KDTREE_DEVICE_DEFAULTS",
           "kdtree_device_scratch_bytes", "PersistentBvhParams", "PersistentBvhResult", "persistent_bvh_params",
           "persistent_bvh_build", "persistent_bvh_scratch_bytes", "PERSISTENT_BVH_DEFAULTS", "SahDeviceResult",
           "sah_device_build", "sah_device_scratch_bytes", "BvhRefitResult", "bvh_refit",
           "bvh_refit_scratch_bytes", "BvhOptimizeResult", "BvhSahResult", "bvh_optimize", "bvh_optimize_scratch_bytes",
           "bvh_sah_cost", "BvhReorderResult", "bvh_reorder", "bvh_reorder_scratch_bytes",
           "PlocResult", "ploc_build", "ploc_scratch_bytes", "PLOC_TAIL", "PLOC_TILE",
           "PlocBatchMesh", "PlocBatchMeshResult", "PlocBatchResult", "ploc_batch_capacity", "ploc_build_batch", "ploc_batch_scratch_bytes",
           "RefitBatchEntry", "BvhRefitBatchResult", "bvh_refit_batch", "bvh_refit_batch_scratch_bytes",
           "INSTANCE_DTYPE", "BlasRange", "BlasPool", "TlasResult", "instance_invert", "make_instances", "tlas_capacity", "tlas_build",
           "tlas_scratch_bytes", "trace_instanced", "InstanceVisibility", "InstancedTraceStats",
           "trace_instanced_masked", "trace_instanced_stats", "TlasRefitResult", "tlas_refit", "tlas_refit_scratch_bytes",
           "BlasTris", "BLAS_TRIS_DTYPE", "InstancedGeometry", "instanced_hit_attributes", "raygen_ao_normals",
           "BvhWideResult", "bvh_widen_capacity", "bvh_widen", "bvh_widen_scratch_bytes", "trace_wide", "trace_wide_stats",
           "WideBlasRange", "TlasWideResult", "InstancedWideTraceStats", "pool_widen_capacity", "pool_widen", "tlas_widen",
           "pool_widen_batch", "pool_widen_batch_scratch_bytes",
           "BvhOptimizeBatchEntry", "BvhOptimizeBatchResult", "BvhSahBatchResult", "bvh_optimize_batch", "bvh_optimize_batch_scratch_bytes",
           "bvh_sah_cost_batch", "OPT_ERR_LINK", "OPT_ERR_ROW", "OPT_ERR_NO_TREE",
           "trace_instanced_wide", "trace_instanced_wide_stats",
           "instanced_validate", "instanced_flags_read", "trace_instanced_fast", "trace_instanced_fast_stats", "InstancedFastStats",
           "instanced_wide_validate", "trace_instanced_wide_fast", "trace_instanced_wide_fast_stats",
           "trace_instanced_seeded", "trace_instanced_seeded_stats", "trace_instanced_wide_seeded", "trace_instanced_wide_seeded_stats",
           "WideRefitEntry", "WideRefitResult", "pool_wide_refit", "pool_wide_refit_scratch_bytes", "tlas_wide_refit",
           "tlas_wide_refit_scratch_bytes",
           "InstancesUpdateResult", "instances_update", "instances_status_read", "instances_update_host", "INSTANCE_MAX_CHAIN",
           "INSTANCE_ERR_SINGULAR", "INSTANCE_ERR_CHAIN",
           "TlasMotionRefitResult", "InstanceMotion", "InstancedMotionStats", "tlas_motion_refit", "tlas_motion_refit_scratch_bytes",
           "trace_instanced_motion", "trace_instanced_motion_stats", "instanced_hit_attributes_motion", "ray_times_primary",
           "ray_times_secondary"]
