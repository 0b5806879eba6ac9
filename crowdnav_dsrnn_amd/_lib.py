"""ctypes binding of the native HIP library (include/crowdnav.h).

The product path has NO fallback: if lib/libcrowdnav_hip.so is missing or fails to load, every entry
point raises. Build it with `python -m crowdnav_dsrnn_amd.build` (or __graft_entry__.build()).

SIGNATURES is the one Python copy of the header's prototypes; tests/test_abi.py compares it with
include/crowdnav.h type by type. The struct mirrors live in abi.py.
"""
import ctypes
import os

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CN_LIB_PATH") or os.path.join(HERE, "lib", "libcrowdnav_hip.so")

_lib = None

# the struct mirrors and their flag, under the names callers use (_lib.GruSeqFwd, ...)
GruSeqFwd, GruSeqBwd, GruStepSeg = abi.GruSeqFwd, abi.GruSeqBwd, abi.GruStepSeg
RolloutOut, RolloutNoise, RolloutLidar = abi.RolloutOut, abi.RolloutNoise, abi.RolloutLidar
ROLLOUT_OBS_EVERY_STEP = abi.ROLLOUT_OBS_EVERY_STEP
DwaParams = abi.DwaParams   # cn_dwa_params

P = ctypes.POINTER
vp, cstr, i32, i64, ll = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_longlong
f32, f64 = ctypes.c_float, ctypes.c_double
cfgp, outp, noisep = P(abi.CnConfig), P(RolloutOut), P(RolloutNoise)

# name -> (restype, argtypes): one entry per prototype of include/crowdnav.h, in its order. `int` is i32; arrays
# and opaque handles (device pointers, streams, the engine) are vp.
SIGNATURES = {
    "cn_last_error": (cstr, []),
    "cn_version": (cstr, []),
    "cn_config_validate": (i32, [cfgp]),
    "cn_create": (i32, [cfgp, i32, P(vp)]),
    "cn_destroy": (None, [vp]),
    "cn_create_mixed": (i32, [cfgp, i32, vp, i64, i32, P(vp)]),
    "cn_env_humans": (i32, [vp, vp]),
    "cn_mixed_scripted": (i32, [vp, i32]),
    "cn_scripted_unicycle": (i32, [vp, i32]),
    "cn_reset": (i32, [vp, vp, vp, vp, vp]),
    "cn_step": (i32, [vp, vp, vp] + [vp] * 9),
    "cn_step_seq": (i32, [vp, vp, i32, vp, i64] + [vp] * 9),
    "cn_set_graph_mode": (i32, [vp, vp, i32]),
    "cn_graph_node_counts": (i32, [vp, P(i64), i32, P(i64)]),
    "cn_state_bytes": (i32, [vp, P(i64)]),
    "cn_state_layout_offsets": (i32, [cfgp, P(i64), P(i64)]),
    "cn_state_field_info": (i32, [i32, P(cstr), P(i32), P(i32)]),
    "cn_get_state": (i32, [vp, vp, vp, i32]),
    "cn_set_state": (i32, [vp, vp, vp, i32]),
    "cn_state_device_ptr": (vp, [vp]),
    "cn_profile": (i32, [vp, i32, i32]),
    "cn_profile_read": (i32, [vp, P(f64), P(f64), P(i64)]),
    "cn_edge_features": (i32, [vp, i64, i32] + [vp] * 14),
    "cn_gru_fwd_step": (i32, [vp, i64, i32] + [vp] * 7),
    "cn_gru_fwd_step_scatter": (i32, [vp, i64, i32] + [vp] * 8 + [i64, i64]),
    "cn_gru_fwd_fused": (i32, [vp, i64, i32] + [vp] * 9 + [i64, i64]),
    "cn_gru_bwd_step": (i32, [vp, i64, i32] + [vp] * 7),
    "cn_gru_bias_blocks": (i64, [i64]),
    "cn_gru_bwd_step_bias": (i32, [vp, i64, i32] + [vp] * 8),
    "cn_gru_bwd_step_gates": (i32, [vp, i64, i32] + [vp] * 7),
    "cn_gru_bias_work_elems": (i64, [i32]),
    "cn_gru_bias_reduce": (i32, [vp, i64, i32] + [vp] * 4),
    "cn_gaussian_act": (i32, [vp, i64, i32] + [vp] * 5),
    "cn_lattice_act": (i32, [vp, i64] + [vp] * 5),
    "cn_lattice_eval_fwd": (i32, [vp, i64] + [vp] * 5),
    "cn_lattice_eval_bwd": (i32, [vp, i64] + [vp] * 5),
    "cn_lattice_soft_fwd": (i32, [vp, i64, vp, vp, f32, vp, vp, vp]),
    "cn_lattice_soft_bwd": (i32, [vp, i64, vp, vp, f32, vp, vp]),
    "cn_gru_fwd_step_group": (i32, [vp, i32, i32, P(GruStepSeg)]),
    "cn_gae": (i32, [vp, i32, i64, f32, f32, i32] + [vp] * 5),
    "cn_gru_fwd_seq": (i32, [vp, i32, i32, i32, P(GruSeqFwd)]),
    "cn_gru_bwd_seq_work_elems": (i64, [i32, i32, i32, P(GruSeqBwd)]),
    "cn_gru_bwd_seq": (i32, [vp, i32, i32, i32, P(GruSeqBwd), vp, i64]),
    "cn_lidar_obs": (i32, [vp, vp, vp, i32, i32, f64, f64, vp, vp]),
    "cn_lidar_scan": (i32, [vp, vp, i32, f64, f64, vp]),
    "cn_debug_disc_quad": (i32, [vp, i64, i32] + [vp] * 6),
    "cn_debug_orca": (i32, [vp, i64, i32, vp, vp, f32, f32, f32, vp]),
    "cn_orca_predict": (i32, [vp, i64, i32, vp, vp, f32, f32, f32, vp]),
    "cn_orca_predict_kd": (i32, [vp, i64, i32, vp, vp, f32, f32, f32, vp, vp]),
    "cn_social_force_predict": (i32, [vp, i64, i32, vp, vp] + [f64] * 4 + [vp]),
    "cn_dwa_predict": (i32, [vp, i64, i32, vp, vp, vp, f64, P(DwaParams), vp, vp, vp]),
    "cn_robot_act": (i32, [vp, vp, i32, vp]),
    "cn_scripted_dwa": (i32, [vp, P(DwaParams)]),
    "cn_mix_ctl_set": (i32, [vp, vp, P(abi.CnMixCtl)]),
    "cn_robot_mix": (i32, [vp, vp, i32, vp, vp, i32, vp, vp, vp]),
    "cn_robot_act_regret": (i32, [vp, vp, i32, vp, vp]),
    "cn_robot_mix_regret": (i32, [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]),
    "cn_visible_mask": (i32, [vp, vp, vp]),
    "cn_rollout": (i32, [vp, vp, i32, i32, outp, P(i32)]),
    "cn_rollout_noisy": (i32, [vp, vp, i32, i32, outp, noisep, P(i32)]),
    "cn_rollout_lidar": (i32, [vp, vp, i32, i32, outp, noisep, P(RolloutLidar), P(i32)]),
    "cn_rollout_masked": (i32, [vp, vp, i32, i32, outp, noisep, vp, P(i32)]),
    "cn_debug_set_spawn_budget": (i32, [vp, ll]),
    "cn_debug_spawn_stats": (i32, [vp, vp]),
    "cn_debug_set_seq_chunk": (i32, [vp, i32]),
    "cn_debug_copy64": (i32, [vp, i64, i32, vp, vp]),
    "cn_attn_pool_fwd": (i32, [vp, i64, i32, i32] + [vp] * 3),
    "cn_attn_pool_bwd": (i32, [vp, i64, i32, i32] + [vp] * 5),
    "cn_spatial_attn_fwd": (i32, [vp, i64, i32, i32, f32] + [vp] * 5),
    "cn_spatial_attn_bwd": (i32, [vp, i64, i32, i32, f32] + [vp] * 7 + [i64, vp, i64]),
    "cn_spatial_attn_var_fwd": (i32, [vp, i64, i32, i32] + [vp] * 7),
    "cn_spatial_attn_var_bwd": (i32, [vp, i64, i32, i32] + [vp] * 9 + [i64, vp, i64]),
    "cn_spatial_attn_mask_fwd": (i32, [vp, i64, i32, i32] + [vp] * 7),
    "cn_spatial_attn_mask_bwd": (i32, [vp, i64, i32, i32] + [vp] * 9 + [i64, vp, i64]),
    "cn_wgrad_work_elems": (i64, [i64, i32, i32]),
    "cn_wgrad": (i32, [vp, i64, i32, i32] + [vp] * 6),
}
EXPORTED = list(SIGNATURES)


class NativeLibraryMissing(RuntimeError):
    pass


class StaleNativeLibrary(NativeLibraryMissing):
    """The library on disk was not built from the sources on disk (embedded CN_SRC_HASH differs)."""


def _check_provenance(L):
    """cn_version() carries the sha256 of the sources the library was built from (build.py). When the
    sources are present (always in-tree, on the GPU box too) they must hash to the same value."""
    from . import build

    ver = L.cn_version().decode()
    mark = build.HASH_MARK.decode()
    got = ver.split(mark, 1)[1][:64] if mark in ver else None
    if os.environ.get("CN_LIB_PATH") or not all(os.path.exists(d) for d in build.DEPS):
        return ver
    want = build.source_hash()
    if got != want:
        raise StaleNativeLibrary(
            "%s was built from other sources (embedded %s, sources on disk %s): rebuild with "
            "`python -m crowdnav_dsrnn_amd.build`" % (LIB_PATH, got, want))
    return ver


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            "HIP engine library not built: %s is missing (run `python -m crowdnav_dsrnn_amd.build`)" % LIB_PATH)
    # torch's HIP runtime first: the library's libamdhip64 dependency then binds to the runtime torch already
    # loaded (torch ships its own copy). Loaded the other way round, the process holds two HIP runtimes, the
    # streams and device pointers the host side passes in belong to the other one, and the library's first
    # launch fails with hipErrorNoDevice.
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        # a library named by CN_LIB_PATH (an A/B run beside an older build) may lack a symbol: it stays unbound and
        # calling it raises; the in-tree library must have every one (ctypes' AttributeError names the symbol)
        if os.environ.get("CN_LIB_PATH") and getattr(L, name, None) is None:
            continue
        f = getattr(L, name)
        f.argtypes, f.restype = argtypes, restype
        if name == "cn_version":   # (cn_last_error and cn_version head the table)
            _check_provenance(L)
    _lib = L
    return L


GRAPH_NODE_TYPES = ("kernel", "memcpy", "memset", "host", "graph", "empty", "wait_event", "event_record",
                    "ext_sem_signal", "ext_sem_wait", "mem_alloc", "mem_free", "memcpy_from_symbol",
                    "memcpy_to_symbol")


def graph_node_counts(graph):
    """{node type: count} of a captured hipGraph_t (torch.cuda.CUDAGraph(keep_graph=True).raw_cuda_graph()),
    through cn_graph_node_counts; types with no node are left out. 'total' = all nodes."""
    n = len(GRAPH_NODE_TYPES)
    counts = (ctypes.c_int64 * n)()
    total = ctypes.c_int64()
    check(lib().cn_graph_node_counts(ctypes.c_void_p(graph), counts, n, ctypes.byref(total)))
    out = {GRAPH_NODE_TYPES[k]: int(counts[k]) for k in range(n) if counts[k]}
    out["total"] = int(total.value)
    return out


def check(rc):
    if rc != 0:
        raise RuntimeError("crowdnav native error %d: %s" % (rc, lib().cn_last_error().decode()))
    return rc
