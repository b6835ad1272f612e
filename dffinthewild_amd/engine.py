"""ctypes binding of ``libdffw.so`` (C ABI: ``include/dffw.h``).

This is the only place Python touches the native library.  There is no CPU or PyTorch fallback:
if the shared object is missing the import of this module raises, and every forward runs the
hand-written gfx950 kernels.  PyTorch is used for device memory (inputs, outputs, the workspace
come from its caching allocator) and for the current HIP stream, nothing else.
"""
import ctypes
import os
import threading
import types
from ctypes import POINTER, byref, c_char_p, c_float, c_int, c_int64, c_void_p

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DFFW_LIB_PATH: load another build of the same library (A/B measurements of kernel variants on one box); in-tree by default
LIB_PATH = os.environ.get("DFFW_LIB_PATH") or os.path.join(_HERE, "libdffw.so")

PRECISIONS = {"bf16x3": 0, "fp16": 1, "bf16": 2}
NET_DEPTH = 0   # Depth_Estimation_Network.Network: DFF_net alone
NET_E2E = 1     # End_to_End.Network: alignment network + FOV warp + DFF_net


class DffwError(RuntimeError):
    pass


class _Tensor(ctypes.Structure):
    _fields_ = [("name", c_char_p), ("data", POINTER(c_float)), ("numel", c_int64)]


class _Tap(ctypes.Structure):
    _fields_ = [("name", c_char_p), ("dst", c_void_p), ("numel", c_int64)]


class _Prof(ctypes.Structure):
    _fields_ = [("kernel", c_char_p), ("layer", c_char_p), ("flops", ctypes.c_double), ("bytes", ctypes.c_double),
                ("ms", c_float)]


class AdamTensor(ctypes.Structure):
    """dffw_adam_tensor: one entry of dffw_adam_step's list."""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("numel", c_int64)]


assert ctypes.sizeof(AdamTensor) == 40   # op_adam_step builds the table as an (n, 5) array of 8-byte words


class SimParams(ctypes.Structure):
    """dffw_sim_params (include/dffw.h)."""
    _fields_ = [("pixel_per_meter", ctypes.c_double), ("min_depth", ctypes.c_double), ("max_depth", ctypes.c_double),
                ("min_focus", ctypes.c_double), ("max_focus", ctypes.c_double), ("num_planes", c_int), ("max_radius", c_int)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise DffwError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C dffinthewild_amd/csrc). "
            "dffinthewild_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.dffw_version.restype = c_char_p
    lib.dffw_last_error.restype = c_char_p
    lib.dffw_last_conv_kernel.restype = c_char_p
    lib.dffw_param_count.argtypes = [c_int]
    lib.dffw_param_info.argtypes = [c_int, c_int, POINTER(c_char_p), POINTER(c_int64), POINTER(c_int), POINTER(c_int)]
    lib.dffw_engine_create.argtypes = [c_int, c_int, POINTER(_Tensor), c_int, c_int, POINTER(c_void_p)]
    lib.dffw_engine_destroy.argtypes = [c_void_p]
    lib.dffw_engine_destroy.restype = None
    lib.dffw_engine_precision.argtypes = [c_void_p]
    lib.dffw_engine_update.argtypes = [c_void_p, POINTER(_Tensor), c_int, c_void_p]
    lib.dffw_engine_repack_stats.argtypes = [c_void_p, POINTER(c_int64)]
    lib.dffw_engine_packed_bytes.argtypes = [c_void_p]
    lib.dffw_engine_packed_bytes.restype = c_int64
    lib.dffw_engine_packed_read.argtypes = [c_void_p, c_void_p, c_int64, c_void_p]
    lib.dffw_workspace_bytes.argtypes = [c_void_p, c_int, c_int, c_int, c_int]
    lib.dffw_workspace_bytes.restype = c_int64
    fwd = [c_void_p, c_void_p, c_void_p, POINTER(c_int64), c_int, c_int, c_int, c_int,
           POINTER(c_void_p), c_void_p, c_int64, c_void_p]
    lib.dffw_forward.argtypes = fwd
    lib.dffw_forward_taps.argtypes = fwd + [POINTER(_Tap), c_int]
    lib.dffw_forward_e2e.argtypes = [c_void_p, c_void_p, c_void_p, POINTER(c_int64), c_void_p, c_int, c_int, c_int, c_int,
                                     POINTER(c_void_p), c_void_p, c_void_p, c_int64, c_void_p, POINTER(_Tap), c_int]
    lib.dffw_forward_raw.argtypes = [c_void_p, c_void_p, c_int, POINTER(c_int64), c_int, c_int, c_void_p, POINTER(c_int64), c_int, c_int, c_int,
                                     c_int, POINTER(c_void_p), c_void_p, c_int64, c_void_p]
    lib.dffw_profile_enable.argtypes = [c_void_p, c_int]
    lib.dffw_profile_collect.argtypes = [c_void_p, POINTER(_Prof), c_int]
    lib.dffw_op_conv3d.argtypes = [c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int,
                                   POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int,
                                   POINTER(c_float), POINTER(c_float), c_void_p, c_int, c_void_p, c_void_p]
    lib.dffw_op_conv3d_ex.argtypes = [c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int,
                                      POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int,
                                      POINTER(c_float), POINTER(c_float), c_void_p, c_int, c_void_p, c_void_p, POINTER(c_float), c_void_p, c_void_p]
    lib.dffw_op_pool.argtypes = [c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.dffw_op_pool3.argtypes = [c_int, c_int, c_void_p] + [c_int] * 5 + [c_void_p] * 4
    lib.dffw_op_srd.argtypes = [c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int] + [POINTER(c_float)] * 6 + [c_void_p] * 3
    lib.dffw_op_efd.argtypes = [c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int] + [POINTER(c_float)] * 4 + [c_int, c_void_p, c_void_p]
    lib.dffw_op_of_block.argtypes = [c_int, c_int, c_void_p] + [c_int] * 7 + [POINTER(c_float)] * 5 + [c_void_p] * 2
    lib.dffw_op_head_tail.argtypes = [c_int, c_int, c_void_p] + [c_int] * 5 + [POINTER(c_float)] * 6 + [c_int] + [c_void_p] * 3
    lib.dffw_op_head_front.argtypes = [c_int, c_int, c_void_p] + [c_int] * 5 + [POINTER(c_float)] * 2 + [c_void_p] * 4
    lib.dffw_last_op_kernels.restype = c_char_p
    lib.dffw_op_fov_warp.argtypes = [c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                                     c_void_p, c_void_p, c_void_p]
    lib.dffw_op_regress.argtypes = [c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                    POINTER(c_int64), c_void_p, c_void_p]
    lib.dffw_op_regress_heads.argtypes = [c_int, c_int, POINTER(c_void_p), POINTER(c_int), POINTER(c_int), POINTER(c_void_p), c_int, c_int, c_int, c_int,
                                          c_void_p, POINTER(c_int64), c_int, c_void_p]
    c_u8p = POINTER(ctypes.c_uint8)
    lib.dffw_pack_stack.argtypes = [c_int, c_void_p, c_int, POINTER(c_int64), c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.dffw_augment_stack.argtypes = [c_int, c_void_p, c_int, POINTER(c_int64)] + [c_int] * 6 + [c_void_p, c_int] + [c_void_p] * 6 + \
                                      [c_int, c_float, c_float, c_float, c_void_p]
    lib.dffw_unpack_stack.argtypes = [c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.dffw_colorize.argtypes = [c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p]
    lib.dffw_jet_lut.argtypes = [c_u8p]
    lib.dffw_metrics_scratch_bytes.argtypes = [c_int]
    lib.dffw_metrics_scratch_bytes.restype = c_int64
    lib.dffw_metrics.argtypes = [c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                 c_int64, c_void_p]
    lib.dffw_comm_unique_id.argtypes = [ctypes.c_char_p]
    lib.dffw_comm_init_rank.argtypes = [c_int, c_int, c_int, ctypes.c_char_p, POINTER(c_void_p)]
    lib.dffw_comm_init_all.argtypes = [c_int, POINTER(c_int), POINTER(c_void_p)]
    lib.dffw_comm_destroy.argtypes = [c_void_p]
    lib.dffw_comm_destroy.restype = None
    lib.dffw_comm_rank.argtypes = [c_void_p]
    lib.dffw_comm_size.argtypes = [c_void_p]
    lib.dffw_allgather.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]
    lib.dffw_probe_peaks.argtypes = [c_int, POINTER(c_float), POINTER(c_float), c_void_p]
    lib.dffw_sim_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int, c_int]
    lib.dffw_sim_workspace_bytes.restype = c_int64
    lib.dffw_sim_render.argtypes = [c_int, SimParams, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int] + [c_void_p] * 7 + [c_int64, c_void_p]
    lib.dffw_sim_plan_host.argtypes = [POINTER(SimParams), POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_double, c_int,
                                       POINTER(ctypes.c_double), POINTER(c_int), POINTER(ctypes.c_double), POINTER(ctypes.c_double), POINTER(c_int)]
    lib.dffw_sim_disk_rows.argtypes = [c_int, POINTER(c_int)]
    lib.dffw_loss_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int]
    lib.dffw_loss_workspace_bytes.restype = c_int64
    lib.dffw_loss_heads.argtypes = [c_int, c_int, POINTER(c_void_p), POINTER(c_int), POINTER(c_int), c_int, c_int, c_int, c_int, c_void_p, POINTER(c_int64),
                                    c_void_p, c_void_p, c_void_p, POINTER(c_float), c_int, c_float, c_float, POINTER(c_void_p), POINTER(c_void_p),
                                    c_void_p, c_void_p, c_int64, c_void_p]
    lib.dffw_heads_backward.argtypes = [c_int, c_int, POINTER(c_void_p), POINTER(c_int), POINTER(c_int), c_int, c_int, c_int, c_int, c_void_p, POINTER(c_int64),
                                        POINTER(c_void_p), POINTER(c_void_p), c_void_p]
    lib.dffw_op_conv3d_backward.argtypes = [c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int,
                                            POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.dffw_conv_wgrad_workspace_bytes.argtypes = [c_int] * 6 + [POINTER(c_int)] * 3 + [c_int]
    lib.dffw_conv_wgrad_workspace_bytes.restype = c_int64
    lib.dffw_conv_wgrad.argtypes = [c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                    POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, c_void_p, c_void_p, c_int64, c_void_p]
    lib.dffw_conv_cat_wgrad_workspace_bytes.argtypes = [c_int] * 7
    lib.dffw_conv_cat_wgrad_workspace_bytes.restype = c_int64
    lib.dffw_conv_cat_wgrad.argtypes = [c_int, c_int, c_void_p, c_int, c_void_p, c_int] + [c_int] * 4 + [c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p]
    lib.dffw_op_conv_cat_backward.argtypes = [c_int, c_int, c_void_p, c_int, c_void_p, c_int] + [c_int] * 4 + [POINTER(c_float), c_int] + [c_void_p] * 5
    lib.dffw_op_conv3d_cat.argtypes = [c_int, c_int, c_void_p, c_int, c_void_p, c_int] + [c_int] * 4 + [POINTER(c_float), c_int, POINTER(c_float), POINTER(c_float),
                                                                                                     c_void_p, c_int, c_void_p, c_void_p]
    c_double = ctypes.c_double
    lib.dffw_bn_train_workspace_bytes.argtypes = [c_int] * 5
    lib.dffw_bn_train_workspace_bytes.restype = c_int64
    lib.dffw_bn_train_forward.argtypes = [c_int, c_int, c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_double, c_double] + [c_void_p] * 3 + \
                                         [c_int] + [c_void_p] * 4 + [c_int64, c_void_p]
    lib.dffw_bn_train_backward.argtypes = [c_int, c_int] + [c_void_p] * 3 + [c_int] * 5 + [c_void_p] * 3 + [c_int] + [c_void_p] * 5 + [c_int64, c_void_p]
    lib.dffw_op_bn_train.argtypes = [c_int, c_int, c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_double, c_double] + [c_void_p] * 3 + \
                                    [c_int] + [c_void_p] * 4
    lib.dffw_op_bn_train_backward.argtypes = [c_int, c_int] + [c_void_p] * 3 + [c_int] * 5 + [c_void_p] * 3 + [c_int] + [c_void_p] * 5
    lib.dffw_op_conv_pw_backward.argtypes = [c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int,
                                             POINTER(c_int), POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p]
    lib.dffw_conv_pw_wgrad_workspace_bytes.argtypes = [c_int] * 6 + [POINTER(c_int)] * 2
    lib.dffw_conv_pw_wgrad_workspace_bytes.restype = c_int64
    lib.dffw_conv_pw_wgrad.argtypes = [c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                       POINTER(c_int), POINTER(c_int), c_void_p, c_void_p, c_int64, c_void_p]
    lib.dffw_att_tail_backward_workspace_bytes.argtypes = [c_int] * 5
    lib.dffw_att_tail_backward_workspace_bytes.restype = c_int64
    lib.dffw_att_tail_backward.argtypes = [c_int, c_int] + [c_void_p] * 4 + [c_int] * 5 + [c_void_p] * 6 + [c_int64, c_void_p]
    lib.dffw_op_att_tail_backward.argtypes = [c_int, c_int] + [c_void_p] * 4 + [c_int] * 5 + [POINTER(c_float)] * 2 + [c_void_p] * 4
    lib.dffw_grad_combine.argtypes = [c_int, c_int] + [c_void_p] * 3 + [c_int] * 5 + [c_void_p] * 2
    lib.dffw_op_grad_combine.argtypes = [c_int, c_int] + [c_void_p] * 3 + [c_int] * 5 + [c_void_p] * 2
    lib.dffw_pool_backward.argtypes = [c_int] * 4 + [c_void_p] * 3 + [c_int] * 5 + [c_void_p] * 2
    lib.dffw_op_pool_backward.argtypes = [c_int] * 4 + [c_void_p] * 3 + [c_int] * 5 + [c_void_p] * 2
    lib.dffw_pool3_backward.argtypes = [c_int, c_int] + [c_void_p] * 4 + [c_int] * 5 + [c_void_p] * 2
    lib.dffw_op_pool3_backward.argtypes = [c_int, c_int] + [c_void_p] * 4 + [c_int] * 5 + [c_void_p] * 2
    lib.dffw_stem_wgrad_workspace_bytes.argtypes = [c_int] * 4
    lib.dffw_stem_wgrad_workspace_bytes.restype = c_int64
    lib.dffw_stem_wgrad.argtypes = [c_int, c_int, c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, c_void_p, c_int64, c_void_p]
    lib.dffw_op_stem_backward.argtypes = [c_int, c_int, c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, c_void_p]
    lib.dffw_score_conv_dgrad.argtypes = [c_int, c_int, c_void_p] + [c_int] * 5 + [c_void_p, POINTER(c_int), POINTER(c_int)] + [c_void_p] * 3
    lib.dffw_score_conv_wgrad_workspace_bytes.argtypes = [c_int] * 5 + [POINTER(c_int)] * 2
    lib.dffw_score_conv_wgrad_workspace_bytes.restype = c_int64
    lib.dffw_score_conv_wgrad.argtypes = [c_int, c_int, c_void_p, c_void_p] + [c_int] * 5 + [POINTER(c_int), POINTER(c_int), c_void_p, c_void_p, c_int64, c_void_p]
    lib.dffw_op_score_conv_backward.argtypes = [c_int, c_int, c_void_p] + [c_int] * 5 + [c_void_p, POINTER(c_int), POINTER(c_int)] + [c_void_p] * 5
    lib.dffw_adam_tensors_per_launch.argtypes = []
    lib.dffw_adam_step.argtypes = [c_int, POINTER(AdamTensor), c_int, c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_void_p]
    return lib


lib = _load()
ADAM_TENSORS_PER_LAUNCH = lib.dffw_adam_tensors_per_launch()   # tensors one launch of dffw_adam_step takes; a longer list takes several launches
COMM_ID_BYTES = 128
RAW_NORM_F64 = 16   # DFFW_RAW_NORM_F64: the FS6 loader's float64 normalisation
AUG_NPARAMS = 8     # DFFW_AUG_NPARAMS: crop row, crop col, contrast, brightness, gamma, flip_x, flip_y, angle

# every symbol include/dffw.h declares (tests check the library exports each one)
ABI_SYMBOLS = (
    "dffw_version", "dffw_last_error", "dffw_param_count", "dffw_param_info", "dffw_engine_create",
    "dffw_engine_destroy", "dffw_engine_precision", "dffw_workspace_bytes", "dffw_forward",
    "dffw_forward_taps", "dffw_profile_enable", "dffw_profile_collect", "dffw_op_conv3d", "dffw_op_conv3d_ex", "dffw_op_pool", "dffw_op_pool3", "dffw_op_regress",
    "dffw_op_regress_heads",
    "dffw_op_fov_warp", "dffw_forward_e2e", "dffw_last_conv_kernel", "dffw_op_srd", "dffw_op_efd", "dffw_last_op_kernels",
    "dffw_op_of_block", "dffw_op_head_tail", "dffw_op_head_front",
    "dffw_forward_raw", "dffw_pack_stack", "dffw_augment_stack", "dffw_unpack_stack", "dffw_colorize", "dffw_jet_lut", "dffw_metrics_scratch_bytes", "dffw_metrics",
    "dffw_comm_unique_id", "dffw_comm_init_rank", "dffw_comm_init_all", "dffw_comm_destroy", "dffw_comm_rank", "dffw_comm_size",
    "dffw_allgather", "dffw_comm_group_start", "dffw_comm_group_end", "dffw_probe_peaks",
    "dffw_sim_workspace_bytes", "dffw_sim_render", "dffw_sim_plan_host", "dffw_sim_disk_rows",
    "dffw_loss_workspace_bytes", "dffw_loss_heads",
    "dffw_op_conv3d_backward", "dffw_conv_wgrad_workspace_bytes", "dffw_conv_wgrad",
    "dffw_bn_train_workspace_bytes", "dffw_bn_train_forward", "dffw_bn_train_backward", "dffw_op_bn_train", "dffw_op_bn_train_backward",
    "dffw_op_conv_pw_backward", "dffw_conv_pw_wgrad_workspace_bytes", "dffw_conv_pw_wgrad", "dffw_grad_combine", "dffw_op_grad_combine",
    "dffw_pool_backward", "dffw_pool3_backward", "dffw_op_pool_backward", "dffw_op_pool3_backward",
    "dffw_stem_wgrad_workspace_bytes", "dffw_stem_wgrad", "dffw_op_stem_backward",
    "dffw_score_conv_dgrad", "dffw_score_conv_wgrad_workspace_bytes", "dffw_score_conv_wgrad", "dffw_op_score_conv_backward",
    "dffw_adam_tensors_per_launch", "dffw_adam_step",
    "dffw_conv_cat_wgrad_workspace_bytes", "dffw_conv_cat_wgrad", "dffw_op_conv_cat_backward", "dffw_op_conv3d_cat",
    "dffw_heads_backward",
    "dffw_att_tail_backward_workspace_bytes", "dffw_att_tail_backward", "dffw_op_att_tail_backward",
    "dffw_engine_update", "dffw_engine_repack_stats", "dffw_engine_packed_bytes", "dffw_engine_packed_read",
)


def _check(rc, what):
    if rc < 0:
        msg = lib.dffw_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise DffwError(f"{what} failed ({rc}): {msg}")
    return rc


def param_table(net=NET_DEPTH):
    """The library's view of the weight contract: list of (key, shape, flags)."""
    n = _check(lib.dffw_param_count(net), "dffw_param_count")
    out = []
    for i in range(n):
        name, shape, ndim, flags = c_char_p(), (c_int64 * 5)(), c_int(), c_int()
        _check(lib.dffw_param_info(net, i, byref(name), shape, byref(ndim), byref(flags)), "dffw_param_info")
        out.append((name.value.decode(), tuple(shape[:ndim.value]), flags.value))
    return out


def _stream_ptr(device):
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _f32(t):
    return ctypes.cast(t.data_ptr(), POINTER(c_float))


def _dev(t):
    """Index of the GPU that holds the tensor ``t``."""
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def _ptr(t):
    """``t``'s device address as a C pointer argument; NULL for None."""
    return c_void_p(t.data_ptr()) if t is not None else None


class Engine:
    """Owns one ``dffw_engine`` (packed weights on one GPU).  Thread-compatible: calls on engines
    of different devices may run concurrently (ctypes releases the GIL)."""

    def __init__(self, state_dict, device, precision="bf16x3", net=NET_DEPTH):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise DffwError("the HIP engine needs a GPU device (no CPU fallback)")
        self.index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.precision = precision
        keep, arr = [], (_Tensor * len(state_dict))()
        i = 0
        for key, t in state_dict.items():
            if not torch.is_floating_point(t):
                continue  # num_batches_tracked counters carry no arithmetic
            h = t.detach().to("cpu", torch.float32).contiguous()
            keep.append(h)
            arr[i] = _Tensor(key.encode(), _f32(h), h.numel())
            i += 1
        self._h = c_void_p()
        _check(lib.dffw_engine_create(self.index, net, arr, i, PRECISIONS[precision], byref(self._h)), "dffw_engine_create")
        self._ws = {}
        self._ws_stream = None      # torch stream the cached workspace was last used on
        self._upd_stream = None     # torch stream of an update() that no forward has been ordered behind yet
        self._lock = threading.Lock()

    # an Engine owns a dffw_engine* and a device workspace: a second owner would free the handle twice
    def __copy__(self):
        raise TypeError("dffinthewild_amd.engine.Engine cannot be copied: build a new one from the state dict")

    def __deepcopy__(self, memo):
        raise TypeError("dffinthewild_amd.engine.Engine cannot be copied: build a new one from the state dict")

    def __reduce__(self):
        raise TypeError("dffinthewild_amd.engine.Engine cannot be pickled: save the model's state_dict instead")

    def __del__(self, _destroy=lib.dffw_engine_destroy):
        h = getattr(self, "_h", None)
        if h:
            _destroy(h)
            self._h = None

    def profile(self, on=True):
        """Bracket every kernel launch of the following forwards with HIP events (bench.py)."""
        _check(lib.dffw_profile_enable(self._h, int(on)), "dffw_profile_enable")

    def profile_collect(self):
        """[(kernel, layer, flops, bytes, ms)] for the launches of the last profiled forward."""
        n = _check(lib.dffw_profile_collect(self._h, None, 0), "dffw_profile_collect")
        arr = (_Prof * n)()
        _check(lib.dffw_profile_collect(self._h, arr, n), "dffw_profile_collect")
        return [(e.kernel.decode(), e.layer.decode(), e.flops, e.bytes, e.ms) for e in arr]

    def workspace_bytes(self, B, N, H, W):
        return _check(lib.dffw_workspace_bytes(self._h, B, N, H, W), "dffw_workspace_bytes")

    def _workspace(self, B, N, H, W, extra=0):
        key = (B, N, H, W, extra)
        ws = self._ws.get(key)
        if ws is None:
            nbytes = self.workspace_bytes(B, N, H, W) + extra
            self._ws.clear()  # one resident workspace: shapes change rarely (test.py runs one dataset per process)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    def _call_ws(self, B, N, H, W, extra, call):
        """Run ``call(ws)`` (a C-ABI forward returning its status) on the cached workspace.  The size is cached per shape, but
        the engine's allocation path also depends on its DFFW_* switches (read per call): if it reports the workspace too
        small (-3) the size is asked for again under the present switches and the forward repeated once."""
        cur = torch.cuda.current_stream(self.index)
        self._after_update(cur)
        if self._ws_stream is not None and self._ws_stream != cur and self._ws:
            # the workspace is one buffer shared by successive forwards: a forward issued under another torch stream must
            # not start before the previous one (on the old stream) is done with it
            ev = torch.cuda.Event()
            ev.record(self._ws_stream)
            cur.wait_event(ev)
        self._ws_stream = cur
        rc = call(self._workspace(B, N, H, W, extra))
        if rc == -3:
            # kernels of the failed attempt (main and internal side streams were joined by the engine) may still be running:
            # let them finish before the block goes back to the allocator
            cur.synchronize()
            self._ws.clear()
            rc = call(self._workspace(B, N, H, W, extra))
        return rc

    def _after_update(self, cur):
        """A forward issued under another torch stream than the last update() must not read the packed weights before the repack kernels
        have written them."""
        if self._upd_stream is not None and self._upd_stream != cur:
            ev = torch.cuda.Event()
            ev.record(self._upd_stream)
            cur.wait_event(ev)
        self._upd_stream = None

    def update(self, state_dict):
        """Repack the weights from ``state_dict`` (the module's own tensors after ``optimizer.step()`` or an in-place edit) on the GPU:
        dffw_engine_update folds BatchNorm and rewrites every operand buffer by two kernels on the current stream, bit for bit what a new
        ``Engine(state_dict)`` would hold.  Every floating entry must be a contiguous float32 CUDA tensor on this engine's device (no host
        round trip, no silent copy): anything else raises.  Enqueue-only after the first call, which builds the engine's repack plan."""
        keep, arr = [], (_Tensor * len(state_dict))()
        i = 0
        for key, t in state_dict.items():
            if not torch.is_tensor(t):
                raise ValueError(f"Engine.update: '{key}' is not a tensor")
            if not torch.is_floating_point(t):
                continue  # num_batches_tracked counters carry no arithmetic
            if not t.is_cuda or _dev(t) != self.index:
                raise ValueError(f"Engine.update: '{key}' is on {t.device}, the engine repacks from tensors on cuda:{self.index} "
                                 "(build a new Engine from a CPU state dict)")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"Engine.update: '{key}' must be a contiguous float32 tensor, got {t.dtype}"
                                 f"{'' if t.is_contiguous() else ' (not contiguous)'}")
            t = t.detach()
            keep.append(t)
            arr[i] = _Tensor(key.encode(), _f32(t), t.numel())
            i += 1
        with self._lock, torch.cuda.device(self.index):
            cur = torch.cuda.current_stream(self.index)
            if self._ws_stream is not None and self._ws_stream != cur:
                # the last forward (on the old stream) may still read the buffers this call rewrites
                ev = torch.cuda.Event()
                ev.record(self._ws_stream)
                cur.wait_event(ev)
            self._after_update(cur)
            _check(lib.dffw_engine_update(self._h, arr, i, _stream_ptr(self.index)), "dffw_engine_update")
            self._upd_stream = cur
            if cur != torch.cuda.default_stream(self.index):
                for t in keep:   # the kernels read the tensors when the stream gets to them: the caching allocator must not hand their memory on before
                    t.record_stream(cur)

    def repack_stats(self):
        """{plan_bytes, fold_bytes, map_bytes, buffer_bytes} of the repack plan (it exists after the first update())."""
        out = (c_int64 * 4)()
        _check(lib.dffw_engine_repack_stats(self._h, out), "dffw_engine_repack_stats")
        return dict(zip(("plan_bytes", "fold_bytes", "map_bytes", "buffer_bytes"), out))

    def packed_bytes(self):
        """Every packed device buffer of the engine, concatenated in a fixed order (layer name, then packing order), as a uint8 CPU tensor
        (tests compare an updated engine with a newly built one)."""
        with self._lock, torch.cuda.device(self.index):
            torch.cuda.synchronize(self.index)
            n = _check(lib.dffw_engine_packed_bytes(self._h), "dffw_engine_packed_bytes")
            out = torch.empty(n, dtype=torch.uint8)
            _check(lib.dffw_engine_packed_read(self._h, c_void_p(out.data_ptr()), n, _stream_ptr(self.index)), "dffw_engine_packed_read")
        return out

    def forward(self, FS, focus_dists, taps=None):
        """FS (B,3,N,H,W) float32 on this engine's device; focus_dists broadcastable to (B,N,H,W).
        Returns (mid_out, pred1, pred2, pred3); with ``taps`` (list of names) also a dict of
        intermediate volumes in the reference's layout."""
        B, C, N, H, W = FS.shape
        FS = FS.contiguous()
        fd = focus_dists.expand(B, N, H, W)
        strides = (c_int64 * 4)(*fd.stride())
        outs = [torch.empty((B, H, W), dtype=torch.float32, device=FS.device) for _ in range(4)]
        optrs = (c_void_p * 4)(*[o.data_ptr() for o in outs])
        with self._lock, torch.cuda.device(self.index):
            def args(ws):
                return [self._h, _ptr(FS), _ptr(fd), strides, B, N, H, W, optrs, _ptr(ws), ws.numel(), _stream_ptr(self.index)]
            if not taps:
                _check(self._call_ws(B, N, H, W, 0, lambda ws: lib.dffw_forward(*args(ws))), "dffw_forward")
                return tuple(outs)
            shapes = _tap_shapes(B, N, H, W)
            bufs = {nm: torch.empty(shapes[nm], dtype=torch.float32, device=FS.device) for nm in taps}
            tarr = (_Tap * len(bufs))(*[_Tap(nm.encode(), _ptr(t), t.numel()) for nm, t in bufs.items()])
            _check(self._call_ws(B, N, H, W, 0, lambda ws: lib.dffw_forward_taps(*args(ws), tarr, len(bufs))), "dffw_forward_taps")
            return tuple(outs), bufs


    def forward_raw(self, raw, strides, dtype, h, w, focus_dists, B, N, H, W):
        """dffw_forward_raw: the stem normalises and pads the raw (uint8 / 0..255 float32) stack on the fly.
        raw: tensor whose storage holds the stack; strides: element strides (sample, slice, row, col, channel) and the
        data pointer already points at the crop origin; H, W: padded sizes."""
        fd = focus_dists.expand(B, N, H, W)
        fst = (c_int64 * 4)(*fd.stride())
        outs = [torch.empty((B, H, W), dtype=torch.float32, device=fd.device) for _ in range(4)]
        optrs = (c_void_p * 4)(*[o.data_ptr() for o in outs])
        with self._lock, torch.cuda.device(self.index):
            st5 = (c_int64 * 5)(*strides)
            _check(self._call_ws(B, N, H, W, B * 3 * N * H * W * 4 + 256,
                                 lambda ws: lib.dffw_forward_raw(self._h, c_void_p(raw), dtype, st5, h, w, _ptr(fd), fst,
                                                                 B, N, H, W, optrs, _ptr(ws), ws.numel(), _stream_ptr(self.index))),
                   "dffw_forward_raw")
        return tuple(outs)

    def forward_e2e(self, FS, focus_dists, fovs, taps=None):
        """End_to_End.Network.forward: FS (B,3,10,H,W), focus_dists broadcastable to (B,10,H,W), fovs with B*10
        elements in (sample, slice) order.  Returns (mid_out, pred1, pred2, pred3, aligned FS); with ``taps``
        also a dict of intermediate values (head3/head2/head1/alpha as (B,3,N), plus the DFF_net taps)."""
        B, C, N, H, W = FS.shape
        FS = FS.contiguous()
        fd = focus_dists.expand(B, N, H, W)
        fov = fovs.reshape(B, N).contiguous()
        strides = (c_int64 * 4)(*fd.stride())
        outs = [torch.empty((B, H, W), dtype=torch.float32, device=FS.device) for _ in range(4)]
        aligned = torch.empty_like(FS)
        optrs = (c_void_p * 4)(*[o.data_ptr() for o in outs])
        with self._lock, torch.cuda.device(self.index):
            bufs, tarr, nt = {}, None, 0
            if taps:
                shapes = _tap_shapes(B, N, H, W)
                bufs = {nm: torch.empty(shapes[nm], dtype=torch.float32, device=FS.device) for nm in taps}
                tarr = (_Tap * len(bufs))(*[_Tap(nm.encode(), _ptr(t), t.numel()) for nm, t in bufs.items()])
                nt = len(bufs)
            _check(self._call_ws(B, N, H, W, 0,
                                 lambda ws: lib.dffw_forward_e2e(self._h, _ptr(FS), _ptr(fd), strides, _ptr(fov), B, N, H, W, optrs, _ptr(aligned),
                                                                 _ptr(ws), ws.numel(), _stream_ptr(self.index), tarr, nt)),
                   "dffw_forward_e2e")
        res = tuple(outs) + (aligned,)
        return (res, bufs) if taps else res


def _tap_shapes(B, N, H, W):
    return {
        "head3": (B, 3, N), "head2": (B, 3, N), "head1": (B, 3, N), "alpha": (B, 3, N),
        "alpha3": (B, 3, N), "alpha2": (B, 3, N),
        "fe1": (B, 8, N, H, W), "fe2": (B, 16, N, H // 2, W // 2), "fe3": (B, 32, N, H // 4, W // 4),
        "stem": (B, 8, N, H, W), "V1": (B, 8, N, H, W), "E1": (B, 16, N, H // 2, W // 2), "V2": (B, 16, N, H // 2, W // 2),
        "E2": (B, 32, N, H // 4, W // 4), "V3": (B, 32, N, H // 4, W // 4),
        "FS_volume": (B, 32, N, H // 8, W // 8), "conf": (B, N, H // 8, W // 8),
        "cost1": (B, N, H // 4, W // 4), "cost2": (B, N, H // 2, W // 2), "cost3": (B, N, H, W),
    }


# ---- single-operator wrappers (used by the kernel parity tests) ----------------------------------
def _i3(v):
    v = (v, v, v) if isinstance(v, int) else tuple(v)
    return (c_int * 3)(*v)


def op_conv3d(x, weight, *, stride=1, pad=0, dilation=1, transposed=False, bn=None, bias=None,
              residual=None, relu=0, precision="bf16x3", want_pre=False, cls_weight=None):
    """y = [relu](BN(conv(x)) [+ residual]) through the MFMA implicit-GEMM kernel.  ``x`` (B,C,N,H,W)
    float32 on the GPU; ``weight`` CPU/GPU float32 in PyTorch layout; ``bn`` = (gamma, beta, mean, var).
    ``want_pre`` / ``cls_weight`` (dffw_op_conv3d_ex): also return BN(conv(x)) before the residual add and / or the scores
    of a bias-free 1x1x1 Cout -> 1 classifier applied to y (the hourglass's last layer, DEN.py:96-97): the result is then
    the tuple (y, y_pre or None, scores or None)."""
    B, Cin, N, H, W = x.shape
    w = weight.detach().to("cpu", torch.float32).contiguous()
    Cout = w.shape[1] if transposed else w.shape[0]
    k = tuple(w.shape[2:])
    s, p, d = _i3(stride), _i3(pad), _i3(dilation)
    if transposed:
        No, Ho, Wo = N, 2 * H, 2 * W
    else:
        No = N + 2 * p[0] - (k[0] - 1)
        Ho = (H + 2 * p[1] - d[1] * (k[1] - 1) - 1) // s[1] + 1
        Wo = (W + 2 * p[2] - d[2] * (k[2] - 1) - 1) // s[2] + 1
    bnh = None
    if bn is not None:
        bnh = torch.cat([t.detach().to("cpu", torch.float32).reshape(-1) for t in bn]).contiguous()
    bh = bias.detach().to("cpu", torch.float32).contiguous() if bias is not None else None
    y = torch.empty((B, No, Ho, Wo) if Cout == 1 else (B, Cout, No, Ho, Wo), dtype=torch.float32, device=x.device)
    x = x.contiguous()
    res = residual.contiguous() if residual is not None else None
    dev = _dev(x)
    ex = want_pre or cls_weight is not None
    y_pre = torch.empty_like(y) if want_pre else None
    cw = cls_weight.detach().to("cpu", torch.float32).reshape(-1).contiguous() if cls_weight is not None else None
    score = torch.empty((B, No, Ho, Wo), dtype=torch.float32, device=x.device) if cw is not None else None
    with torch.cuda.device(dev):
        args = (dev, PRECISIONS[precision], _ptr(x), B, Cin, N, H, W, _f32(w), Cout,
                (c_int * 3)(*k), s, p, d, int(transposed),
                _f32(bnh) if bnh is not None else None, _f32(bh) if bh is not None else None, _ptr(res), relu, _ptr(y))
        if ex:
            _check(lib.dffw_op_conv3d_ex(*args, _ptr(y_pre), _f32(cw) if cw is not None else None, _ptr(score), _stream_ptr(dev)), "dffw_op_conv3d_ex")
            return y, y_pre, score
        _check(lib.dffw_op_conv3d(*args, _stream_ptr(dev)), "dffw_op_conv3d")
    return y


def conv3d_output_shape(x_shape, weight_shape, stride, pad, transposed):
    """Shape of conv(x, weight) for the plain convs of op_conv3d_backward (dilation 1; the transposed form has output_padding (0,1,1))."""
    B, Cin, N, H, W = x_shape
    k, s, p = tuple(weight_shape[2:]), tuple(_i3(stride)), tuple(_i3(pad))
    if transposed:
        return (B, weight_shape[1], N, 2 * H, 2 * W)
    return (B, weight_shape[0], N + 2 * p[0] - (k[0] - 1), (H + 2 * p[1] - k[1]) // s[1] + 1, (W + 2 * p[2] - k[2]) // s[2] + 1)


def _conv_backward(fn, x, weight, grad, need, precision, *, checks, layout, want, what, b=None, weight_on_gpu=False):
    """The body the (grad_x, grad_w) wrappers share.  ``fn``: the C entry point, whose name less ``dffw_`` is the wrapper's.  ``checks``: the
    wrapper's own argument checks, in order, each a callable that returns a message (-> ValueError) or None.  ``layout(t)``: the C arguments
    between the precision and the stream, from the pointers ``t.x, t.w, t.grad, t.b, t.gx, t.gw`` and the shape ``t.B, t.Cin, t.N, t.H, t.W``.
    ``want()``: the shape ``grad`` (``what`` it is, for the message) must have; it is compared after the library's own refusals."""
    name = fn.__name__[len("dffw_"):]
    if any(t.device.type != "cuda" for t in (x, grad, b) if t is not None):
        raise DffwError(f"{name} needs GPU tensors (no CPU fallback)")
    for check in checks:
        msg = check()
        if msg:
            raise ValueError(f"{name}: {msg}")
    w = weight.detach().to(x.device if weight_on_gpu else "cpu", torch.float32).contiguous()
    x, grad, b = (t.detach().float().contiguous() if t is not None else None for t in (x, grad, b))
    dev = _dev(x)
    gx = torch.empty_like(x) if "x" in need else None
    gw = torch.empty(tuple(w.shape), dtype=torch.float32, device=x.device) if "w" in need else None
    B, Cin, N, H, W = x.shape

    def call(with_x, with_w):
        t = types.SimpleNamespace(x=_ptr(x), w=_ptr(w) if weight_on_gpu else _f32(w), grad=_ptr(grad), b=_ptr(b) if with_x else None,
                                  gx=_ptr(gx) if with_x else None, gw=_ptr(gw) if with_w else None, B=B, Cin=Cin, N=N, H=H, W=W)
        return fn(dev, PRECISIONS[precision], *layout(t), _stream_ptr(dev))
    with torch.cuda.device(dev):
        # the C entry point's own refusals first (a call with no output launches nothing), then the gradient's shape
        _check(call(False, False), fn.__name__)
        if tuple(grad.shape) != want():
            raise ValueError(f"{name}: {what[0]} {tuple(grad.shape)} is not the {what[1]} {want()}")
        _check(call(gx is not None, gw is not None), fn.__name__)
    return gx, gw


def op_conv3d_backward(x, weight, grad_y, *, stride=1, pad=0, dilation=1, transposed=False, precision="bf16x3", need=("x", "w")):
    """(grad_x, grad_w) of <grad_y, conv(x, weight)> for the plain convs of the aggregation network (dffw_op_conv3d_backward: 3x3x3 and 1x3x3
    stride 1, 3x3x3 stride (1,2,2), the transposed 3x3x3; no BN, bias, ReLU or residual).  ``x`` (B,Cin,N,H,W) and ``grad_y`` float32 on the
    GPU, ``weight`` CPU/GPU float32 in PyTorch layout.  ``need``: which of "x", "w" to compute; the other entry is None.  grad_x comes from the
    adjoint conv through the forward's dispatch, grad_w from the conv_wgrad kernels; both are float32 GPU tensors."""
    checks = (lambda: tuple(_i3(dilation)) != (1, 1, 1) and f"dilation must be 1, got {dilation}",
              lambda: (x.dim() != 5 or weight.dim() != 5 or grad_y.dim() != 5) and "x, weight and grad_y must have 5 dimensions",
              lambda: weight.shape[0 if transposed else 1] != x.shape[1] and f"weight {tuple(weight.shape)} does not take {x.shape[1]} input channels")
    return _conv_backward(
        lib.dffw_op_conv3d_backward, x, weight, grad_y, need, precision, checks=checks,
        layout=lambda t: (t.x, t.B, t.Cin, t.N, t.H, t.W, t.w, weight.shape[1 if transposed else 0], _i3(weight.shape[2:]), _i3(stride), _i3(pad),
                          int(transposed), t.grad, t.gx, t.gw),
        want=lambda: conv3d_output_shape(x.shape, weight.shape, stride, pad, transposed), what=("grad_y", "conv's output shape"))


def op_conv_pw_backward(x, weight, grad_y, *, pad, stride=1, dilation=1, precision="bf16x3", need=("x", "w")):
    """(grad_x, grad_w) of <grad_y, conv(x, weight)> for the convs without in-plane taps (dffw_op_conv_pw_backward): kernel
    (3,1,1) with pad (1,0,0) and kernel (1,1,1) with pad 0, stride 1, no bias; channels multiples of 8 up to 128.  ``x`` (B,Cin,N,H,W) and
    ``grad_y`` (B,Cout,N,H,W) float32 on the GPU, ``weight`` CPU/GPU float32 (Cout,Cin,kd,1,1); ``stride`` and ``dilation`` must be 1.  ``need``: which of "x", "w" to compute; the
    other entry is None.  grad_x comes from the adjoint conv through the forward's dispatch, grad_w from the conv_pw_wgrad kernels."""
    checks = (lambda: (tuple(_i3(stride)) != (1, 1, 1) or tuple(_i3(dilation)) != (1, 1, 1)) and f"stride and dilation must be 1, got {stride} and {dilation}",
              lambda: (x.dim() != 5 or weight.dim() != 5 or grad_y.dim() != 5) and "x, weight and grad_y must have 5 dimensions",
              lambda: weight.shape[1] != x.shape[1] and f"weight {tuple(weight.shape)} does not take {x.shape[1]} input channels")
    return _conv_backward(
        lib.dffw_op_conv_pw_backward, x, weight, grad_y, need, precision, checks=checks,
        layout=lambda t: (t.x, t.B, t.Cin, t.N, t.H, t.W, t.w, weight.shape[0], _i3(weight.shape[2:]), _i3(pad), t.grad, t.gx, t.gw),
        want=lambda: (x.shape[0], weight.shape[0]) + tuple(x.shape[2:]), what=("grad_y", "conv's output shape"))   # the conv's output has x's volume


def op_conv_cat_backward(xa, xb, weight, grad_y, *, precision="bf16x3", need=("xa", "xb", "w")):
    """(grad_xa, grad_xb, grad_w) of <grad_y, conv(cat([xa, xb], 1), weight)> for the convs whose input is a channel concatenation
    (dffw_op_conv_cat_backward): kernel (3,3,3), stride 1, pad 1, no bias; ``xa`` (B,Ca,N,H,W), ``xb`` (B,Cb,N,H,W) and
    ``grad_y`` (B,Cout,N,H,W) float32 on the GPU, ``weight`` CPU/GPU float32 (Cout,Ca+Cb,3,3,3); Ca, Cb, Cout multiples of 8 from 8 to 128,
    Ca + Cb <= 192.  ``need``: which of "xa", "xb", "w" to compute; the other entries are None.  grad_xa / grad_xb are two adjoint convs on the
    weight's slices through the forward's dispatch, grad_w comes from the conv_wgrad_cat kernels; the concatenation is never built."""
    name = "op_conv_cat_backward"
    # the shapes first (they need no GPU), then the device; the channel counts' limits are the library's to refuse
    checks = (lambda: any(t.dim() != 5 for t in (xa, xb, weight, grad_y)) and "xa, xb, weight and grad_y must have 5 dimensions",
              lambda: (xa.shape[0], *xa.shape[2:]) != (xb.shape[0], *xb.shape[2:]) and
              f"xa {tuple(xa.shape)} and xb {tuple(xb.shape)} differ outside the channel axis",
              lambda: tuple(weight.shape[2:]) != (3, 3, 3) and f"the conv over a concatenation is 3x3x3 stride 1 pad 1, got a {tuple(weight.shape[2:])} kernel",
              lambda: weight.shape[1] != xa.shape[1] + xb.shape[1] and
              f"weight {tuple(weight.shape)} does not take {xa.shape[1]} + {xb.shape[1]} input channels",
              lambda: tuple(grad_y.shape) != (xa.shape[0], weight.shape[0], *xa.shape[2:]) and
              f"grad_y {tuple(grad_y.shape)} is not the conv's output shape {(xa.shape[0], weight.shape[0], *xa.shape[2:])}",
              lambda: set(need) - {"xa", "xb", "w"} and f"need {tuple(need)} names something other than 'xa', 'xb', 'w'")
    for check in checks:
        msg = check()
        if msg:
            raise ValueError(f"{name}: {msg}")
    if any(t.device.type != "cuda" for t in (xa, xb, grad_y)):
        raise DffwError(f"{name} needs GPU tensors (no CPU fallback)")
    if len({t.device for t in (xa, xb, grad_y)}) != 1:
        raise ValueError(f"{name}: xa, xb and grad_y must be on one GPU")
    w = weight.detach().to("cpu", torch.float32).contiguous()
    xa, xb, grad_y = (t.detach().float().contiguous() for t in (xa, xb, grad_y))
    dev = _dev(xa)
    B, Ca, N, H, W = xa.shape
    Cb, Cout = xb.shape[1], w.shape[0]
    gxa = torch.empty_like(xa) if "xa" in need else None
    gxb = torch.empty_like(xb) if "xb" in need else None
    gw = torch.empty(tuple(w.shape), dtype=torch.float32, device=xa.device) if "w" in need else None
    with torch.cuda.device(dev):
        _check(lib.dffw_op_conv_cat_backward(dev, PRECISIONS[precision], _ptr(xa), Ca, _ptr(xb), Cb, B, N, H, W, _f32(w), Cout, _ptr(grad_y), _ptr(gxa),
                                             _ptr(gxb), _ptr(gw), _stream_ptr(dev)), "dffw_op_conv_cat_backward")
    return gxa, gxb, gw


def op_conv3d_cat(xa, xb, weight, *, bn=None, bias=None, residual=None, relu=0, precision="bf16x3"):
    """y = [relu](BN(conv3d(cat([xa, xb], 1), weight)) [+ residual]) with the concatenation left virtual (dffw_op_conv3d_cat, DESIGN.md section
    26): kernel (3,3,3), stride 1, pad 1; ``xa`` (B,Ca,N,H,W), ``xb`` (B,Cb,N,H,W) and ``residual`` (B,Cout,N,H,W) float32 on the GPU, ``weight``
    CPU/GPU float32 (Cout,Ca+Cb,3,3,3); ``bn``, ``bias`` and ``relu`` as op_conv3d takes them.  The forward's dispatch picks the kernel, whose
    fill reads the two tensors; last_conv_kernel() names it.  The channel counts' limits are the library's to refuse."""
    name = "op_conv3d_cat"
    checks = (lambda: any(t.dim() != 5 for t in (xa, xb, weight)) and "xa, xb and weight must have 5 dimensions",
              lambda: (xa.shape[0], *xa.shape[2:]) != (xb.shape[0], *xb.shape[2:]) and
              f"xa {tuple(xa.shape)} and xb {tuple(xb.shape)} differ outside the channel axis",
              lambda: tuple(weight.shape[2:]) != (3, 3, 3) and f"the conv over a concatenation is 3x3x3 stride 1 pad 1, got a {tuple(weight.shape[2:])} kernel",
              lambda: weight.shape[1] != xa.shape[1] + xb.shape[1] and
              f"weight {tuple(weight.shape)} does not take {xa.shape[1]} + {xb.shape[1]} input channels",
              lambda: residual is not None and tuple(residual.shape) != (xa.shape[0], weight.shape[0], *xa.shape[2:]) and
              f"residual {tuple(residual.shape)} is not the conv's output shape {(xa.shape[0], weight.shape[0], *xa.shape[2:])}")
    for check in checks:
        msg = check()
        if msg:
            raise ValueError(f"{name}: {msg}")
    tensors = [t for t in (xa, xb, residual) if t is not None]
    if any(t.device.type != "cuda" for t in tensors):
        raise DffwError(f"{name} needs GPU tensors (no CPU fallback)")
    if len({t.device for t in tensors}) != 1:
        raise ValueError(f"{name}: xa, xb and residual must be on one GPU")
    w = _host_f32(weight)
    xa, xb = (t.detach().float().contiguous() for t in (xa, xb))
    res = residual.detach().float().contiguous() if residual is not None else None
    bnh = _bn_host(bn) if bn is not None else None
    bh = _host_f32(bias) if bias is not None else None
    dev = _dev(xa)
    B, Ca, N, H, W = xa.shape
    Cb, Cout = xb.shape[1], w.shape[0]
    y = torch.empty((B, Cout, N, H, W), dtype=torch.float32, device=xa.device)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_conv3d_cat(dev, PRECISIONS[precision], _ptr(xa), Ca, _ptr(xb), Cb, B, N, H, W, _f32(w), Cout, _f32(bnh) if bnh is not None else None,
                                      _f32(bh) if bh is not None else None, _ptr(res), relu, _ptr(y), _stream_ptr(dev)), "dffw_op_conv3d_cat")
    return y


def op_grad_combine(a, y=None, b=None, *, precision="bf16x3"):
    """``[y > 0] * a (+ b)`` on the activation records of ``precision`` (dffw_op_grad_combine): the ReLU mask of a conv that
    has no BatchNorm, taken from the stored output ``y``, and / or the sum of two gradients of one tensor.  ``a``, ``y``, ``b`` (B,C,N,H,W)
    float32 on the GPU, C a multiple of 8 up to 128; ``y`` and ``b`` may each be None, not both."""
    tensors = [a] + [t for t in (y, b) if t is not None]
    if any(t.device.type != "cuda" for t in tensors):
        raise DffwError("op_grad_combine needs GPU tensors (no CPU fallback)")
    if a.dim() != 5 or any(t.shape != a.shape for t in tensors):
        raise ValueError("op_grad_combine: a, y and b must be 5-dimensional tensors of one shape")
    if y is None and b is None:
        raise ValueError("op_grad_combine: neither a mask (y) nor a second gradient (b): a copy is no operation")
    B, C, N, H, W = a.shape
    a, y, b = (t.detach().float().contiguous() if t is not None else None for t in (a, y, b))
    dev = _dev(a)
    out = torch.empty_like(a)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_grad_combine(dev, PRECISIONS[precision], _ptr(a), _ptr(y), _ptr(b), B, C, N, H, W, _ptr(out), _stream_ptr(dev)),
               "dffw_op_grad_combine")
    return out


def op_attention_tail(x, w3, w1, *, precision="bf16x3"):
    """The attention tail of a Feature_Extraction block, ``y = x + relu(conv111(relu(conv311(x))))``, as the three steps
    that define it: ``a = op_conv3d(x, w3, pad=(1,0,0), relu=1)``, ``t = op_conv3d(a, w1, relu=1)``, ``y = x + t`` in fp32.  Returns (y, a, t);
    ``a`` and ``t`` are what op_attention_tail_backward reads its masks from."""
    a = op_conv3d(x, w3, pad=(1, 0, 0), relu=1, precision=precision)
    t = op_conv3d(a, w1, relu=1, precision=precision)
    return x + t, a, t


def op_attention_tail_backward(x, a, t, grad_y, w3, w1, *, precision="bf16x3", need=("x", "w")):
    """(grad_x, grad_w3, grad_w1) of <grad_y, x + relu(conv111(relu(conv311(x))))> in one kernel (dffw_op_att_tail_backward).
    ``x``, ``a``, ``t`` (op_attention_tail's) and ``grad_y`` (B,C,N,H,W) float32 on the GPU, C = 8, 16 or 32; ``w3`` (C,C,3,1,1) and ``w1``
    (C,C,1,1,1) CPU/GPU float32.  The ReLU masks are those of the stored ``a`` and ``t``.  ``need``: which of "x", "w" to compute ("w": both
    weight gradients); the other entries are None."""
    name = "op_attention_tail_backward"
    tensors = (x, a, t, grad_y)
    if any(v.device.type != "cuda" for v in tensors):
        raise DffwError(f"{name} needs GPU tensors (no CPU fallback)")
    if x.dim() != 5 or any(v.shape != x.shape for v in tensors):
        raise ValueError(f"{name}: x, a, t and grad_y must be 5-dimensional tensors of one shape")
    B, C, N, H, W = x.shape
    if tuple(w3.shape) != (C, C, 3, 1, 1) or tuple(w1.shape) != (C, C, 1, 1, 1):
        raise ValueError(f"{name}: w3 {tuple(w3.shape)} and w1 {tuple(w1.shape)} are not ({C},{C},3,1,1) and ({C},{C},1,1,1)")
    if set(need) - {"x", "w"}:
        raise ValueError(f"{name}: need {tuple(need)} names something other than 'x', 'w'")
    x, a, t, grad_y = (v.detach().float().contiguous() for v in tensors)
    w3h, w1h = _host_f32(w3), _host_f32(w1)
    dev = _dev(x)
    gx = torch.empty_like(x) if "x" in need else None
    gw3 = torch.empty((C, C, 3, 1, 1), dtype=torch.float32, device=x.device) if "w" in need else None
    gw1 = torch.empty((C, C, 1, 1, 1), dtype=torch.float32, device=x.device) if "w" in need else None
    with torch.cuda.device(dev):
        _check(lib.dffw_op_att_tail_backward(dev, PRECISIONS[precision], _ptr(x), _ptr(a), _ptr(t), _ptr(grad_y), B, C, N, H, W, _f32(w3h), _f32(w1h),
                                             _ptr(gx), _ptr(gw3), _ptr(gw1), _stream_ptr(dev)), "dffw_op_att_tail_backward")
    return gx, gw3, gw1


POOL_MODES = {"max": 0, "avg": 1}   # dffw_op_pool's and dffw_op_pool_backward's mode


def op_pool_backward(grad_y, x=None, b=None, *, k, mode, precision="bf16x3"):
    """Gradient of the (1,k,k) pool's input on the activation records of ``precision`` (dffw_op_pool_backward).
    ``grad_y`` (B,C,N,H/k,W/k) float32 on the GPU, C a multiple of 8 up to 128.  ``mode`` "max" (k = 2): ``x`` (B,C,N,H,W), the forward's
    input, names the window's first maximum in row-major order, which receives the gradient.  ``mode`` "avg" (k = 2, 4, 8): every pixel of a
    window receives grad_y / k^2; ``x`` is not needed.  ``b`` (B,C,N,H,W): a second gradient of the input, added in."""
    if mode not in POOL_MODES:
        raise ValueError(f"op_pool_backward: mode must be one of {sorted(POOL_MODES)}, got {mode!r}")
    tensors = [grad_y] + [t for t in (x, b) if t is not None]
    if any(t.device.type != "cuda" for t in tensors):
        raise DffwError("op_pool_backward needs GPU tensors (no CPU fallback)")
    if grad_y.dim() != 5:
        raise ValueError("op_pool_backward: grad_y must have 5 dimensions")
    B, C, N, Ho, Wo = grad_y.shape
    k = int(k)
    shape = (B, C, N, Ho * k, Wo * k)
    for t, what in ((x, "x"), (b, "b")):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"op_pool_backward: {what} {tuple(t.shape)} is not the pool's input shape {shape}")
    grad_y, x, b = (t.detach().float().contiguous() if t is not None else None for t in (grad_y, x, b))
    dev = _dev(grad_y)
    out = torch.empty(shape, dtype=torch.float32, device=grad_y.device)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_pool_backward(dev, PRECISIONS[precision], POOL_MODES[mode], k, _ptr(grad_y), _ptr(x), _ptr(b), B, C, N, shape[3], shape[4],
                                         _ptr(out), _stream_ptr(dev)), "dffw_op_pool_backward")
    return out


def op_pool3_backward(g2, g4, g8, b=None, *, precision="bf16x3"):
    """Gradient of the input of the pyramid's three average pools (1,2,2), (1,4,4), (1,8,8) in one pass (dffw_op_pool3_backward, DESIGN.md
    section 16): ``g2`` (B,C,N,H/2,W/2), ``g4`` (B,C,N,H/4,W/4), ``g8`` (B,C,N,H/8,W/8) float32 on the GPU, the gradients of the three pooled
    volumes; ``b`` (B,C,N,H,W): a second gradient of the input, added in.  Returns ((g8 / 64 + g4 / 16) + g2 / 4) (+ b) at (B,C,N,H,W)."""
    tensors = [g2, g4, g8] + ([b] if b is not None else [])
    if any(t is None for t in tensors):
        raise ValueError("op_pool3_backward needs all of g2, g4 and g8")
    if any(t.device.type != "cuda" for t in tensors):
        raise DffwError("op_pool3_backward needs GPU tensors (no CPU fallback)")
    if g8.dim() != 5:
        raise ValueError("op_pool3_backward: g8 must have 5 dimensions")
    B, C, N, H8, W8 = g8.shape
    shape = (B, C, N, 8 * H8, 8 * W8)
    for t, what, f in ((g2, "g2", 4), (g4, "g4", 2), (b, "b", None)):
        want = shape if f is None else (B, C, N, f * H8, f * W8)
        if t is not None and tuple(t.shape) != want:
            raise ValueError(f"op_pool3_backward: {what} {tuple(t.shape)} does not go with g8 {tuple(g8.shape)}: expected {want}")
    g2, g4, g8, b = (t.detach().float().contiguous() if t is not None else None for t in (g2, g4, g8, b))
    dev = _dev(g8)
    out = torch.empty(shape, dtype=torch.float32, device=g8.device)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_pool3_backward(dev, PRECISIONS[precision], _ptr(g2), _ptr(g4), _ptr(g8), _ptr(b), B, C, N, shape[3], shape[4], _ptr(out),
                                          _stream_ptr(dev)), "dffw_op_pool3_backward")
    return out


def op_score_conv_backward(x, weight, grad_score, *, pad, b=None, precision="bf16x3", need=("x", "w")):
    """(grad_x, grad_w) of <grad_score, conv(x, weight)> for the convs that produce the score volumes (dffw_op_score_conv_backward, DESIGN.md
    section 19): one output channel, kernel (1,1,1) with pad 0 or kernel (3,3,3) with pad 1, stride 1, no bias; Cin a multiple of 8 up to 128.
    ``x`` (B,Cin,N,h,w) float32 on the GPU, ``grad_score`` (B,N,h,w) float32 on the GPU, as the loss heads write it: it stays fp32.  ``weight``
    CPU/GPU float32 (1,Cin,k,k,k).  ``b`` (B,Cin,N,h,w): a second gradient of ``x``, added into grad_x.  ``need``: which of "x", "w" to
    compute; the other entry is None.  Both come from the score_dgrad / score_wgrad kernels; grad_x is a record value of ``precision``."""
    checks = (lambda: (x.dim() != 5 or weight.dim() != 5) and "x and weight must have 5 dimensions",
              lambda: weight.shape[0] != 1 and f"weight {tuple(weight.shape)} has {weight.shape[0]} output channels, a score conv has one",
              lambda: weight.shape[1] != x.shape[1] and f"weight {tuple(weight.shape)} does not take {x.shape[1]} input channels",
              lambda: b is not None and tuple(b.shape) != tuple(x.shape) and f"b {tuple(b.shape)} is not x's shape {tuple(x.shape)}",
              lambda: b is not None and "x" not in need and "b is added to grad_x, which is not asked for")
    return _conv_backward(
        lib.dffw_op_score_conv_backward, x, weight, grad_score, need, precision, checks=checks, b=b, weight_on_gpu=True,
        layout=lambda t: (t.x, t.B, t.Cin, t.N, t.H, t.W, t.w, _i3(weight.shape[2:]), _i3(pad), t.grad, t.b, t.gx, t.gw),
        want=lambda: (x.shape[0],) + tuple(x.shape[2:]), what=("grad_score", "score volume's shape"))   # the score volume of x


STEM_WEIGHT_SHAPE = (8, 3, 1, 9, 9)   # FM_measure.Focus_extraction.0.0: Conv3d(3, 8, (1,9,9), pad (0,8,8), dilation (1,2,2), bias=False)
STEM_GEOMETRY = dict(stride=1, pad=(0, 8, 8), dilation=(1, 2, 2))


def op_stem_backward(x, grad_y, *, precision="bf16x3"):
    """grad_w (8,3,1,9,9) of <grad_y, stem(x, w)> for the stem, the dilated 1x9x9 conv of the image stack (dffw_op_stem_backward, DESIGN.md
    section 17): ``x`` (B,3,N,H,W) and ``grad_y`` (B,8,N,H,W) float32 on the GPU.  The result is a float32 GPU tensor from the stem_wgrad
    kernels.  The stem's input is the image: there is no grad_x."""
    if x.device.type != "cuda" or grad_y.device.type != "cuda":
        raise DffwError("op_stem_backward needs GPU tensors (no CPU fallback)")
    if x.dim() != 5 or grad_y.dim() != 5:
        raise ValueError("op_stem_backward: x and grad_y must have 5 dimensions")
    B, Cin, N, H, W = x.shape
    if Cin != STEM_WEIGHT_SHAPE[1]:
        raise ValueError(f"op_stem_backward: x {tuple(x.shape)} does not have the stem's 3 input channels")
    want = (B, STEM_WEIGHT_SHAPE[0], N, H, W)
    if tuple(grad_y.shape) != want:
        raise ValueError(f"op_stem_backward: grad_y {tuple(grad_y.shape)} is not the stem's output shape {want}")
    x, grad_y = x.detach().float().contiguous(), grad_y.detach().float().contiguous()
    dev = _dev(x)
    gw = torch.empty(STEM_WEIGHT_SHAPE, dtype=torch.float32, device=x.device)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_stem_backward(dev, PRECISIONS[precision], _ptr(x), _ptr(grad_y), B, N, H, W, _ptr(gw), _stream_ptr(dev)),
               "dffw_op_stem_backward")
    return gw


BN_EPS = 1e-5   # nn.BatchNorm3d's default, the value every BatchNorm of the reference network has


def _bn_vec(t, C, dev, what):
    if t.device.type != "cuda":
        raise DffwError(f"{what} must be a GPU tensor (no CPU fallback)")
    if t.numel() != C:
        raise ValueError(f"{what} holds {t.numel()} values, the tensor has {C} channels")
    return t.detach().to(dev, torch.float32).contiguous()


def op_bn_train(x, gamma, beta, running_mean=None, running_var=None, *, residual=None, relu=False, eps=BN_EPS, momentum=0.1, precision="bf16x3"):
    """Train-mode BatchNorm3d (dffw_op_bn_train): ``y = [relu](gamma (x - mean) invstd + beta [+ residual])`` with the batch
    statistics of ``x`` (B,C,N,H,W) float32 on the GPU, C in {8, 16, 32, 64, 128}.  Returns (y, save_mean, save_invstd); ``running_mean`` /
    ``running_var`` (float32 GPU tensors of C values) are updated in place with ``momentum`` (unbiased variance), as nn.BatchNorm3d does."""
    tensors = [x, gamma, beta] + [t for t in (running_mean, running_var, residual) if t is not None]
    if any(t.device.type != "cuda" for t in tensors):
        raise DffwError("op_bn_train needs GPU tensors (no CPU fallback)")
    if x.dim() != 5:
        raise ValueError("op_bn_train: x must have 5 dimensions")
    B, C, N, H, W = x.shape
    if residual is not None and residual.shape != x.shape:
        raise ValueError(f"op_bn_train: residual {tuple(residual.shape)} is not x's shape {tuple(x.shape)}")
    for t in (running_mean, running_var):
        if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == C and t.device == x.device):
            raise ValueError("op_bn_train: the running statistics must be contiguous float32 tensors of C values on x's device (they are updated in place)")
    x = x.detach().float().contiguous()
    res = residual.detach().float().contiguous() if residual is not None else None
    g, b = _bn_vec(gamma, C, x.device, "gamma"), _bn_vec(beta, C, x.device, "beta")
    dev = _dev(x)
    y = torch.empty_like(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty_like(mean)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_bn_train(dev, PRECISIONS[precision], _ptr(x), B, C, N, H, W, _ptr(g), _ptr(b), float(eps), float(momentum), _ptr(running_mean),
                                    _ptr(running_var), _ptr(res), int(bool(relu)), _ptr(y), _ptr(mean), _ptr(invstd), _stream_ptr(dev)), "dffw_op_bn_train")
    return y, mean, invstd


def op_bn_train_backward(x, y, grad_y, gamma, save_mean, save_invstd, *, relu=False, residual=False, precision="bf16x3", need=("x", "params")):
    """Backward of op_bn_train (dffw_op_bn_train_backward): returns (grad_x, grad_res or None, grad_gamma, grad_beta).  ``y`` is the forward's
    output (the ReLU mask is ``y > 0``; may be None without ReLU), ``residual``: whether a residual was added (grad_res is then the masked grad_y).
    ``need`` without "x": only the parameter gradients are computed (grad_x and grad_res come back None); they are always computed."""
    tensors = [x, grad_y, gamma, save_mean, save_invstd] + ([y] if y is not None else [])
    if any(t.device.type != "cuda" for t in tensors):
        raise DffwError("op_bn_train_backward needs GPU tensors (no CPU fallback)")
    if x.dim() != 5 or grad_y.shape != x.shape or (y is not None and y.shape != x.shape):
        raise ValueError("op_bn_train_backward: x, y and grad_y must be 5-dimensional tensors of one shape")
    if relu and y is None:
        raise ValueError("op_bn_train_backward: the ReLU mask is read from y")
    B, C, N, H, W = x.shape
    x, grad_y = x.detach().float().contiguous(), grad_y.detach().float().contiguous()
    y = y.detach().float().contiguous() if relu else None
    g, mean, invstd = (_bn_vec(t, C, x.device, n) for t, n in ((gamma, "gamma"), (save_mean, "save_mean"), (save_invstd, "save_invstd")))
    dev = _dev(x)
    gx = torch.empty_like(x) if "x" in need else None
    gres = torch.empty_like(x) if residual and gx is not None else None
    gg = torch.empty(C, dtype=torch.float32, device=x.device)
    gb = torch.empty_like(gg)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_bn_train_backward(dev, PRECISIONS[precision], _ptr(x), _ptr(y), _ptr(grad_y), B, C, N, H, W, _ptr(g), _ptr(mean), _ptr(invstd),
                                             int(bool(relu)), _ptr(gx), _ptr(gres), _ptr(gg), _ptr(gb), _stream_ptr(dev)), "dffw_op_bn_train_backward")
    return gx, gres, gg, gb


def op_adam_step(params, grads, exp_avgs, exp_avg_sqs, *, step, lr, betas=(0.9, 0.99), eps=1e-8):
    """One Adam step over a whole parameter list in ceil(n / ADAM_TENSORS_PER_LAUNCH) launches (dffw_adam_step): four lists of
    float32 contiguous tensors on ONE GPU, the same shapes position by position.  ``params``, ``exp_avgs`` and ``exp_avg_sqs`` are updated in
    place, ``grads`` are only read; ``step`` is the step count after the increment (1 for the first step).  torch.optim.Adam's arithmetic
    without weight decay, amsgrad or maximize; the betas default to the reference training scripts' (0.9, 0.99).  Enqueue-only on the current
    stream of that GPU: nothing is allocated, copied or waited for."""
    lists = (list(params), list(grads), list(exp_avgs), list(exp_avg_sqs))
    n = len(lists[0])
    if any(len(l) != n for l in lists):
        raise ValueError(f"op_adam_step: the four lists hold {[len(l) for l in lists]} tensors")
    f32, T = torch.float32, torch.Tensor
    try:   # whole lists at a time (a step over 200 tensors is bound by this Python); the loop below finds the offender and words the refusal
        shapes = [t.shape for t in lists[0]]
        good = all({t.dtype for t in l} <= {f32} and all(map(T.is_contiguous, l)) and [t.shape for t in l] == shapes for l in lists)
    except (AttributeError, TypeError):
        good = False
    if not good:
        for what, l in zip(("params", "grads", "exp_avgs", "exp_avg_sqs"), lists):
            for i, t in enumerate(l):
                if not isinstance(t, torch.Tensor) or t.dtype != f32:
                    raise ValueError(f"op_adam_step: {what}[{i}] is not a float32 tensor")
                if not t.is_contiguous():
                    raise ValueError(f"op_adam_step: {what}[{i}] is not contiguous")
                if t.shape != lists[0][i].shape:
                    raise ValueError(f"op_adam_step: {what}[{i}] {tuple(t.shape)} does not have the shape of params[{i}] {tuple(lists[0][i].shape)}")
    devs = set().union(*(map(T.get_device, l) for l in lists))   # -1: a CPU tensor
    if -1 in devs:
        raise DffwError("op_adam_step needs GPU tensors (no CPU fallback)")
    if len(devs) > 1:
        raise ValueError("op_adam_step: the tensors are on more than one GPU (one call per device)")
    b1, b2 = betas
    # dffw_adam_tensor is five 8-byte words: the table is an (n, 5) int64 array
    table = np.empty((n, 5), dtype=np.uint64)
    for k, l in enumerate(lists):
        table[:, k] = np.fromiter(map(T.data_ptr, l), dtype=np.uint64, count=n)
    table[:, 4] = np.fromiter(map(T.numel, lists[0]), dtype=np.uint64, count=n)
    tp = table.ctypes.data_as(POINTER(AdamTensor))
    if not n:   # the library's refusal of an empty list, without a device to name
        _check(lib.dffw_adam_step(0, tp, 0, int(step), float(lr), float(b1), float(b2), float(eps), None), "dffw_adam_step")
        return
    dev = devs.pop()
    with torch.cuda.device(dev):
        _check(lib.dffw_adam_step(dev, tp, n, int(step), float(lr), float(b1), float(b2), float(eps), _stream_ptr(dev)), "dffw_adam_step")


def probe_peaks(device=0):
    """(sustained bf16 MFMA TFLOP/s, sustained HBM copy GB/s) of this GPU, measured now (dffw_probe_peaks)."""
    m, h = c_float(), c_float()
    with torch.cuda.device(device):
        _check(lib.dffw_probe_peaks(device, byref(m), byref(h), _stream_ptr(device)), "dffw_probe_peaks")
    return m.value, h.value


def last_conv_kernel():
    """Kernel instantiation used by this thread's most recent convolution launch (rocprofv3 spelling)."""
    return lib.dffw_last_conv_kernel().decode()


def _host_f32(t):
    return t.detach().to("cpu", torch.float32).contiguous()


def _bn_host(bn):
    return torch.cat([_host_f32(t).reshape(-1) for t in bn]).contiguous()


def op_srd(x, w0, bn0, w2, bn2, w3, w1, *, pooled=False, precision="bf16x3"):
    """One SRD block (dffw_op_srd) through the forward's dispatch: ``x`` (B,C,N,H,W) float32 on the GPU, C = 8, 16 or 32; the
    weights in PyTorch layout, ``bn0`` / ``bn2`` = (gamma, beta, mean, var).  Returns y, or (y, max_pool(1,2,2)(y)) with
    ``pooled``.  op_kernels() then lists the launches."""
    B, C, N, H, W = x.shape
    x = x.contiguous()
    y = torch.empty_like(x)
    pl = torch.empty((B, C, N, H // 2, W // 2), dtype=torch.float32, device=x.device) if pooled else None
    host = [_host_f32(w0), _bn_host(bn0), _host_f32(w2), _bn_host(bn2), _host_f32(w3), _host_f32(w1)]
    dev = _dev(x)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_srd(dev, PRECISIONS[precision], _ptr(x), B, C, N, H, W, *[_f32(t) for t in host], _ptr(y), _ptr(pl), _stream_ptr(dev)), "dffw_op_srd")
    return (y, pl) if pooled else y


def op_efd(x, ws, bns, wp, bnp, *, pooled_at_hand=True, precision="bf16x3"):
    """One EFD block (dffw_op_efd): ``x`` (B,Cin,N,H,W), Cin = 8 or 16, H and W even; returns (B,2*Cin,N,H/2,W/2).  With
    ``pooled_at_hand`` the pooled copy of x is made first and handed to the block, as in the forward."""
    B, C, N, H, W = x.shape
    x = x.contiguous()
    y = torch.empty((B, 2 * C, N, H // 2, W // 2), dtype=torch.float32, device=x.device)
    host = [_host_f32(ws), _bn_host(bns), _host_f32(wp), _bn_host(bnp)]
    dev = _dev(x)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_efd(dev, PRECISIONS[precision], _ptr(x), B, C, N, H, W, *[_f32(t) for t in host],
                               int(bool(pooled_at_hand)), _ptr(y), _stream_ptr(dev)), "dffw_op_efd")
    return y


def op_of_block(x, w0, bn0, w2, bn2, wf, *, stride=1, precision="bf16x3"):
    """One resnet_block_2d_OF of the alignment network (dffw_op_of_block) through the forward's dispatch: ``x`` (B,Cin,N,H,W) float32
    on the GPU (the fp32 stack for the 3 -> 8 first block), weights in PyTorch layout, ``bn0`` / ``bn2`` = (gamma, beta, mean, var),
    ``wf`` the shortcut's 1x1x1 weights.  Returns (B,Cout,N,H/stride,W/stride).  op_kernels() then lists the launches."""
    B, C, N, H, W = x.shape
    Cout = w0.shape[0]
    x = x.contiguous()
    y = torch.empty((B, Cout, N, H // stride, W // stride), dtype=torch.float32, device=x.device)
    host = [_host_f32(w0), _bn_host(bn0), _host_f32(w2), _bn_host(bn2), _host_f32(wf)]
    dev = _dev(x)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_of_block(dev, PRECISIONS[precision], _ptr(x), B, C, N, H, W, Cout, stride,
                                    *[_f32(t) for t in host], _ptr(y), _stream_ptr(dev)), "dffw_op_of_block")
    return y


def op_head_tail(x, w2, bn2, w4, bn4, w6, bias6, alpha, raw, *, start=0, precision="bf16x3"):
    """The back half of one alpha head (dffw_op_head_tail) through the forward's dispatch: ``x`` (B,C,N,H,W) float32 on the GPU, C = 16, 32 or
    64, the head's first-conv output y0 (``start=0``) or its third-conv output y2 (``start=2``); weights in PyTorch layout, ``bn2`` / ``bn4`` =
    (gamma, beta, mean, var).  ``alpha`` and ``raw``: contiguous float32 (B,3,N) GPU tensors; alpha is updated in place (+= the plane means, the
    scale term damped by 0.001), raw receives the undamped means.  op_kernels() then lists the launches."""
    if x.device.type != "cuda" or alpha.device != x.device or raw.device != x.device:
        raise DffwError("op_head_tail needs GPU tensors (no CPU fallback)")
    if x.dim() != 5:
        raise ValueError("op_head_tail: x must have 5 dimensions")
    B, C, N, H, W = x.shape
    for t, what in ((alpha, "alpha"), (raw, "raw")):
        if t.dtype != torch.float32 or tuple(t.shape) != (B, 3, N) or not t.is_contiguous():
            raise ValueError(f"op_head_tail: {what} must be a contiguous float32 ({B},3,{N}) tensor, got {t.dtype} {tuple(t.shape)}")
    x = x.detach().float().contiguous()
    host = [_host_f32(w2), _bn_host(bn2), _host_f32(w4), _bn_host(bn4), _host_f32(w6), _host_f32(bias6)]
    dev = _dev(x)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_head_tail(dev, PRECISIONS[precision], _ptr(x), B, C, N, H, W, *[_f32(t) for t in host], int(start),
                                     _ptr(alpha), _ptr(raw), _stream_ptr(dev)), "dffw_op_head_tail")


def op_head_front(fe, w0, bn0, alpha, fov, *, precision="bf16x3", out=None):
    """The front half of one alpha head (dffw_op_head_front) through the forward's dispatch: ``fe`` (B,C,N,H,W) float32 on the GPU, C = 8, 16 or
    32, the level features; ``w0`` (2C,2C+2,1,3,3) in PyTorch layout with ``bn0`` = (gamma, beta, mean, var); ``alpha`` (B,3,N) and ``fov`` (B,N)
    float32 on the GPU.  Returns y0 = relu(BN(conv([warp(fe)[N-1] | warp(fe)[n] | flow]))), (B,2C,N,H,W), written into ``out`` when given (a
    contiguous float32 GPU tensor of that shape).  op_kernels() then lists the launches."""
    if fe.device.type != "cuda" or alpha.device != fe.device or fov.device != fe.device:
        raise DffwError("op_head_front needs GPU tensors (no CPU fallback)")
    if fe.dim() != 5:
        raise ValueError("op_head_front: fe must have 5 dimensions")
    B, C, N, H, W = fe.shape
    if tuple(w0.shape) != (2 * C, 2 * C + 2, 1, 3, 3):
        raise ValueError(f"op_head_front: w0 must be ({2 * C},{2 * C + 2},1,3,3), got {tuple(w0.shape)}")
    fe = fe.detach().float().contiguous()
    a = alpha.detach().reshape(B, 3, N).float().contiguous()
    f = fov.detach().reshape(B, N).float().contiguous()
    y0 = torch.empty((B, 2 * C, N, H, W), dtype=torch.float32, device=fe.device) if out is None else out
    if y0.dtype != torch.float32 or tuple(y0.shape) != (B, 2 * C, N, H, W) or not y0.is_contiguous() or y0.device != fe.device:
        raise ValueError(f"op_head_front: out must be a contiguous float32 ({B},{2 * C},{N},{H},{W}) tensor on fe's device")
    host = [_host_f32(w0), _bn_host(bn0)]
    dev = _dev(fe)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_head_front(dev, PRECISIONS[precision], _ptr(fe), B, C, N, H, W, *[_f32(t) for t in host], _ptr(a), _ptr(f), _ptr(y0),
                                      _stream_ptr(dev)), "dffw_op_head_front")
    return y0


def op_kernels():
    """Kernel names of every launch of this thread's last op_pool3 / op_srd / op_efd / op_of_block / op_head_front / op_head_tail / op_regress_heads / op_heads_backward
    call, in launch order."""
    s = lib.dffw_last_op_kernels().decode()
    return s.split(";") if s else []


def op_pool(x, k, mode="max", precision="bf16x3"):
    B, C, N, H, W = x.shape
    y = torch.empty((B, C, N, H // k, W // k), dtype=torch.float32, device=x.device)
    x = x.contiguous()
    dev = _dev(x)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_pool(dev, PRECISIONS[precision], 0 if mode == "max" else 1, k, _ptr(x), B, C, N, H, W, _ptr(y), _stream_ptr(dev)), "dffw_op_pool")
    return y


def op_pool3(x, precision="bf16x3"):
    """(p2, p4, p8): the average pools (1,2,2), (1,4,4), (1,8,8) of x (B,C,N,H,W) float32 CUDA, C, H and W multiples of 8, from one pass of the
    forward's dffw::pool3_kernel (dffw_op_pool3; op_kernels() names it), each bit-identical to op_pool(x, k, "avg")."""
    B, C, N, H, W = x.shape
    x = x.contiguous()
    ps = [torch.empty((B, C, N, H // k, W // k), dtype=torch.float32, device=x.device) for k in (2, 4, 8)]
    dev = _dev(x)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_pool3(dev, PRECISIONS[precision], _ptr(x), B, C, N, H, W, *[_ptr(p) for p in ps], _stream_ptr(dev)), "dffw_op_pool3")
    return tuple(ps)


def op_regress(score, focus_dists, H, W):
    B, N, h, w = score.shape
    score = score.contiguous()
    fd = focus_dists.expand(B, N, H, W)
    depth = torch.empty((B, H, W), dtype=torch.float32, device=score.device)
    dev = _dev(score)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_regress(dev, _ptr(score), B, N, h, w, H, W, _ptr(fd), (c_int64 * 4)(*fd.stride()), _ptr(depth), _stream_ptr(dev)),
               "dffw_op_regress")
    return depth


def op_regress_heads(scores, focus_dists, H, W, *, fused=True, out=None):
    """dffw_op_regress_heads: 1..4 regression heads in one launch, as the forward runs them.  scores: fp32 (B,N,h_k,w_k) CUDA tensors;
    focus_dists broadcastable to (B,N,H,W), read through its strides as given (expanded, never copied).  fused=False: regress_kernel whatever
    the shape (the forward under DFFW_NO_REGRESS_FUSED).  out: optional list of contiguous fp32 (B,H,W) tensors to write into.  Returns the
    list of depth maps; op_kernels() then names the kernel launched."""
    n = len(scores)
    if not 1 <= n <= 4:
        raise ValueError(f"op_regress_heads: 1 to 4 heads, got {n}")
    B, N = scores[0].shape[:2]
    device = scores[0].device
    if device.type != "cuda":
        raise DffwError("op_regress_heads needs GPU tensors (no CPU fallback)")
    scores = [s.contiguous() for s in scores]
    for s in scores:
        if s.dtype != torch.float32 or s.dim() != 4 or s.shape[0] != B or s.shape[1] != N:
            raise ValueError(f"score volumes must be float32 (B,N,h,w) with B={B}, N={N}; got {s.dtype} {tuple(s.shape)}")
    if focus_dists.dtype != torch.float32 or focus_dists.device != device:
        raise ValueError("focus_dists must be float32 on the scores' device")
    fd = focus_dists.expand(B, N, H, W)
    if out is None:
        out = [torch.empty((B, H, W), dtype=torch.float32, device=device) for _ in range(n)]
    if len(out) != n or any(o.dtype != torch.float32 or tuple(o.shape) != (B, H, W) or not o.is_contiguous() or o.device != device for o in out):
        raise ValueError(f"out must be {n} contiguous float32 ({B},{H},{W}) tensors on the scores' device")
    dev = _dev(scores[0])
    ptrs = lambda ts: (c_void_p * 4)(*[t.data_ptr() for t in ts])
    with torch.cuda.device(dev):
        _check(lib.dffw_op_regress_heads(dev, n, ptrs(scores), (c_int * 4)(*[s.shape[2] for s in scores]), (c_int * 4)(*[s.shape[3] for s in scores]),
                                         ptrs(out), B, N, H, W, _ptr(fd), (c_int64 * 4)(*fd.stride()), int(bool(fused)), _stream_ptr(dev)),
               "dffw_op_regress_heads")
    return list(out)


def loss_workspace_bytes(B, N, H, W):
    return int(lib.dffw_loss_workspace_bytes(B, N, H, W))


def op_loss_heads(scores, focus_dists, gt, mask, conf=None, weights=(0.3, 0.5, 0.7, 1.0), depth_range=None, *, preds=True, grads=True,
                  workspace=None):
    """dffw_loss_heads: the training scripts' loss over 1..4 regression heads and its gradient down to the score volumes.
    scores: fp32 (B,N,h_k,w_k) CUDA tensors; focus_dists broadcastable to (B,N,H,W); gt fp32 (B,H,W); mask uint8 (B,H,W); conf fp32 (B,H,W)
    or None; depth_range (lo, hi) or None.  preds / grads: False skips those outputs (NULL in the C ABI).  workspace: uint8 tensor of at least
    loss_workspace_bytes(B,N,H,W) (allocated when None; it need not be cleared).
    Returns (losses fp64 (n_heads+1: per head, then the weighted total), [pred_k (B,H,W)] or None, [grad_k like scores[k]] or None)."""
    n = len(scores)
    B, H, W = gt.shape
    N = scores[0].shape[1]
    dev = _dev(scores[0])
    device = scores[0].device
    scores = [s.contiguous() for s in scores]
    for s in scores:
        if s.dtype != torch.float32 or s.dim() != 4 or s.shape[0] != B or s.shape[1] != N:
            raise ValueError(f"score volumes must be float32 (B,N,h,w) with B={B}, N={N}; got {s.dtype} {tuple(s.shape)}")
    gt, mask = gt.contiguous(), mask.contiguous()
    if gt.dtype != torch.float32 or mask.dtype != torch.uint8 or tuple(mask.shape) != (B, H, W):
        raise ValueError("gt must be float32 (B,H,W) and mask uint8 of the same shape")
    if conf is not None:
        conf = conf.contiguous()
        if conf.dtype != torch.float32 or tuple(conf.shape) != (B, H, W):
            raise ValueError("conf must be float32 (B,H,W)")
    if len(weights) < n:
        raise ValueError(f"{n} heads but {len(weights)} weights")
    fd = focus_dists.expand(B, N, H, W)
    pred = [torch.empty((B, H, W), dtype=torch.float32, device=device) for _ in range(n)] if preds else None
    grad = [torch.empty_like(s) for s in scores] if grads else None
    losses = torch.empty(n + 1, dtype=torch.float64, device=device)
    need = loss_workspace_bytes(B, N, H, W)
    ws = workspace if workspace is not None else torch.empty(max(need, 8), dtype=torch.uint8, device=device)
    ptrs = lambda ts: (c_void_p * 4)(*[t.data_ptr() for t in ts]) if ts is not None else None
    lo, hi = (0.0, 1.0) if depth_range is None else (float(depth_range[0]), float(depth_range[1]))
    with torch.cuda.device(dev):
        _check(lib.dffw_loss_heads(dev, n, ptrs(scores), (c_int * 4)(*[s.shape[2] for s in scores]), (c_int * 4)(*[s.shape[3] for s in scores]),
                                   B, N, H, W, _ptr(fd), (c_int64 * 4)(*fd.stride()), _ptr(gt), _ptr(mask), _ptr(conf),
                                   (c_float * 4)(*[float(x) for x in weights[:n]]), 0 if depth_range is None else 1, lo, hi, ptrs(pred), ptrs(grad),
                                   _ptr(losses), _ptr(ws), ws.numel(), _stream_ptr(dev)), "dffw_loss_heads")
    return losses, pred, grad


def op_heads_backward(scores, focus_dists, grad_preds, H, W, *, out=None):
    """dffw_heads_backward: the gradient of 1..4 regression heads (op_regress_heads) under any upstream gradient, down to the score volumes.
    scores: fp32 (B,N,h_k,w_k) CUDA tensors with H = s*h_k, W = s*w_k, s in {1,2,4,8}; focus_dists broadcastable to (B,N,H,W), read through
    its strides; grad_preds[k]: contiguous fp32 (B,H,W), or None for a head without a gradient (not launched).  out: optional list of
    contiguous fp32 tensors shaped like the scores to write into (entries of skipped heads are ignored).  Enqueue-only on the current
    stream.  Returns the list of gradients, None where grad_preds[k] is None; op_kernels() then names the launches."""
    n = len(scores)
    if not 1 <= n <= 4:
        raise ValueError(f"op_heads_backward: 1 to 4 heads, got {n}")
    if len(grad_preds) != n:
        raise ValueError(f"op_heads_backward: {n} heads but {len(grad_preds)} upstream gradients")
    B, N = scores[0].shape[:2]
    device = scores[0].device
    if device.type != "cuda":
        raise DffwError("op_heads_backward needs GPU tensors (no CPU fallback)")
    scores = [s.contiguous() for s in scores]
    for s in scores:
        if s.dtype != torch.float32 or s.dim() != 4 or s.shape[0] != B or s.shape[1] != N:
            raise ValueError(f"score volumes must be float32 (B,N,h,w) with B={B}, N={N}; got {s.dtype} {tuple(s.shape)}")
    if focus_dists.dtype != torch.float32 or focus_dists.device != device:
        raise ValueError("focus_dists must be float32 on the scores' device")
    for g in grad_preds:
        if g is not None and (g.dtype != torch.float32 or tuple(g.shape) != (B, H, W) or not g.is_contiguous() or g.device != device):
            raise ValueError(f"upstream gradients must be contiguous float32 ({B},{H},{W}) tensors on the scores' device")
    fd = focus_dists.expand(B, N, H, W)
    if out is None:
        out = [torch.empty_like(s) if g is not None else None for s, g in zip(scores, grad_preds)]
    else:
        if len(out) != n:
            raise ValueError(f"out must list {n} tensors")
        out = [o if g is not None else None for o, g in zip(out, grad_preds)]
        for o, s in zip(out, scores):
            if o is not None and (o.dtype != torch.float32 or o.shape != s.shape or not o.is_contiguous() or o.device != device):
                raise ValueError("out must be contiguous float32 tensors shaped like the scores, on their device")
    dev = _dev(scores[0])
    ptrs = lambda ts: (c_void_p * 4)(*[t.data_ptr() if t is not None else None for t in ts])
    with torch.cuda.device(dev):
        _check(lib.dffw_heads_backward(dev, n, ptrs(scores), (c_int * 4)(*[s.shape[2] for s in scores]), (c_int * 4)(*[s.shape[3] for s in scores]),
                                       B, N, H, W, _ptr(fd), (c_int64 * 4)(*fd.stride()), ptrs(grad_preds), ptrs(out), _stream_ptr(dev)),
               "dffw_heads_backward")
    return list(out)


def op_fov_warp(x, alpha, fovs, compat_batch_alpha0=False, out=None, flow=None):
    """FlowNetwork.FOV_warp of the reference's End_to_End path (End_to_End.py:106-134) on the GPU.
    x (B,C,N,H,W), alpha (B,3,N,1,1) or (B,3,N), fovs (B,1,N,1,1) or (B,N); returns (warped, flow (B,2,N,H,W)), written into ``out`` /
    ``flow`` when given (contiguous float32 GPU tensors of those shapes)."""
    B, C, N, H, W = x.shape
    x = x.contiguous()
    a = alpha.reshape(B, 3, N).contiguous().float()
    f = fovs.reshape(B, N).contiguous().float()
    out = torch.empty_like(x) if out is None else out
    flow = torch.empty((B, 2, N, H, W), dtype=torch.float32, device=x.device) if flow is None else flow
    for t, shape, what in ((out, (B, C, N, H, W), "out"), (flow, (B, 2, N, H, W), "flow")):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"op_fov_warp: {what} must be a contiguous float32 {shape} tensor on x's device")
    dev = _dev(x)
    with torch.cuda.device(dev):
        _check(lib.dffw_op_fov_warp(dev, _ptr(x), B, C, N, H, W, _ptr(a), _ptr(f), int(compat_batch_alpha0), _ptr(out), _ptr(flow), _stream_ptr(dev)),
               "dffw_op_fov_warp")
    return out, flow


# ---- focal-stack simulator (dffw_sim_*) --------------------------------------------------------------------------------------
SIM_LDS_RADIUS = 32     # DFFW_SIM_LDS_RADIUS
SIM_NSCALARS = 12       # DFFW_SIM_NSCALARS, in this order:
SIM_SCALARS = ("fd", "fd_px", "lens_to_sensor", "fov", "coc_scale", "f_px", "lens_dia", "scene_min", "scene_max", "min_afov",
               "max_afov", "origin_max_afov")


def sim_params(pixel_per_meter, depth_range, focus_range, num_planes, max_radius=-1):
    """dffw_sim_params from (min_depth, max_depth) and (min_focus, max_focus)."""
    return SimParams(float(pixel_per_meter), float(depth_range[0]), float(depth_range[1]), float(focus_range[0]),
                     float(focus_range[1]), int(num_planes), int(max_radius))


def sim_plan_host(params, cam, dmin, dmax, N):
    """dffw_sim_plan_host: per-slice scalars (N, SIM_NSCALARS) and the layer tables [(coc, lo, hi) arrays] of every slice."""
    import numpy as np
    P = params.num_planes
    sc = np.zeros((N, SIM_NSCALARS), np.float64)
    coc = np.zeros((N, P), np.int32)
    lo = np.zeros((N, P), np.float64)
    hi = np.zeros((N, P), np.float64)
    nl = np.zeros(N, np.int32)
    dp = POINTER(ctypes.c_double)
    camv = (ctypes.c_double * 4)(*[float(v) for v in cam])
    _check(lib.dffw_sim_plan_host(byref(params), camv, float(dmin), float(dmax), N, sc.ctypes.data_as(dp),
                                  coc.ctypes.data_as(POINTER(c_int)), lo.ctypes.data_as(dp), hi.ctypes.data_as(dp),
                                  nl.ctypes.data_as(POINTER(c_int))), "dffw_sim_plan_host")
    return sc, [(coc[n, :nl[n]].copy(), lo[n, :nl[n]].copy(), hi[n, :nl[n]].copy()) for n in range(N)]


def sim_disk_rows(r):
    """dffw_sim_disk_rows: half-widths of rows 0..r of the radius-r disk, and the tap count K."""
    hw = (c_int * (r + 1))()
    K = _check(lib.dffw_sim_disk_rows(r, hw), "dffw_sim_disk_rows")
    return list(hw), K


def op_sim_render(image, depth, cams, shifts, params, *, tap=False, workspace=None):
    """dffw_sim_render on the GPU.  image float32 (B,H,W,3) 0..255, depth float64 (B,H,W), cams float64 (B,4), shifts float64
    (B,N,2), all CUDA tensors on one device; params a SimParams.  Returns a dict: images uint8 (B,N,H,W,3), defocus float64
    (B,N,H,W), depth float32 (B,H,W), status int32 (B), slices float64 (B,N,2) (focus distance, FoV), and with ``tap`` the
    warped float image (B,N,H,W,3).  ``workspace``: optional uint8 CUDA tensor of at least sim_workspace_bytes bytes.
    op_kernels() then lists the launches."""
    B, H, W, C = image.shape
    N = shifts.shape[1]
    if C != 3 or tuple(depth.shape) != (B, H, W) or tuple(cams.shape) != (B, 4) or tuple(shifts.shape) != (B, N, 2):
        raise ValueError(f"shapes image {tuple(image.shape)} depth {tuple(depth.shape)} cams {tuple(cams.shape)} shifts {tuple(shifts.shape)}")
    if image.dtype != torch.float32 or depth.dtype != torch.float64 or cams.dtype != torch.float64 or shifts.dtype != torch.float64:
        raise TypeError("image float32, depth / cams / shifts float64")
    dev = image.device
    if dev.type != "cuda" or any(t.device != dev for t in (depth, cams, shifts)):
        raise DffwError("the simulator runs on one GPU: every input must be a CUDA tensor on the same device")
    image, depth, cams, shifts = (t.contiguous() for t in (image, depth, cams, shifts))
    idx = _dev(image)
    need = lib.dffw_sim_workspace_bytes(B, N, H, W, params.num_planes)
    ws = workspace if workspace is not None else torch.empty(need, dtype=torch.uint8, device=dev)
    out = {
        "images": torch.empty((B, N, H, W, 3), dtype=torch.uint8, device=dev),
        "defocus": torch.empty((B, N, H, W), dtype=torch.float64, device=dev),
        "depth": torch.empty((B, H, W), dtype=torch.float32, device=dev),
        "status": torch.empty((B,), dtype=torch.int32, device=dev),
        "slices": torch.empty((B, N, 2), dtype=torch.float64, device=dev),
    }
    if tap:
        out["warped"] = torch.empty((B, N, H, W, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(idx):
        _check(lib.dffw_sim_render(idx, params, _ptr(cams), _ptr(image), _ptr(depth), _ptr(shifts), B, N, H, W,
                                   *[_ptr(out.get(k)) for k in ("images", "defocus", "depth", "status", "slices", "warped")],
                                   _ptr(ws), ws.numel(), _stream_ptr(idx)),
               "dffw_sim_render")
    return out


def sim_workspace_bytes(B, N, H, W, num_planes):
    return int(lib.dffw_sim_workspace_bytes(B, N, H, W, num_planes))
