"""ctypes mirror of the libfpm_hip.so C ABI (include/fpm_hip.h).

This is the Python face of the reference's ``runFPM(FPM_Dataset*)``
(fpmMain.cpp:274): ``Solver`` owns one ``fpm_ctx`` on one GPU and exposes
create / upload / init / run / download with numpy arrays, and ``run_fpm`` is
the one-shot call.  Errors raise ``FpmError`` carrying the library's negative
code and ``fpm_last_error()`` text.  There is no CPU fallback: if the HIP
library cannot be loaded, ``load_library`` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(os.path.dirname(_HERE))          # fpm-opencv_amd/
LIB_DIR = os.path.join(PKG_ROOT, "lib")
# FPM_HIP_LIB: an alternative build of the same library (compiler-flag A/B
# experiments under tools/gpu/); the default is the in-tree build
HIP_LIB = os.environ.get("FPM_HIP_LIB") or os.path.join(LIB_DIR, "libfpm_hip.so")
HOST_LIB = os.path.join(LIB_DIR, "libfpm_host.so")

FPM_OK = 0
FPM_ERR_INVAL = -22
FPM_ERR_NOMEM = -12
FPM_ERR_DEVICE = -5
FPM_ERR_STATE = -71
FPM_ERR_NODEV = -19

PATH_AUTO, PATH_GENERAL, PATH_FUSED = 0, 1, 2
FLAG_OBJCROP_LAST_ONLY = 1
FLAG_SPEC_FP16 = 2          # fp16 spectrum storage, fp32 arithmetic (config 5)
FLAG_SCALAR_RE_ONLY = 4     # legacy: cv::add(UMat c2, double) on the real channel only (fpm_hip.h)
# fpm_set_state flags (fpm_hip.h FPM_STATE_*)
STATE_DEVICE = 1            # objF / pupil are device pointers on the context's device
STATE_PUPIL_SHARED = 2      # one [Np][Np] pupil for every patch
# fpm_stitch / fpm_stitch_tiles flags (fpm_hip.h FPM_STITCH_*)
STITCH_ALIGN_PHASE = 1      # neighbours brought to a common phase
STITCH_ALIGN_COMPLEX = 2    # phase and scale
STITCH_DEVICE = 4           # tiles / field are device pointers
STITCH_ALIGN = {"none": 0, "phase": STITCH_ALIGN_PHASE, "complex": STITCH_ALIGN_COMPLEX}

# fpm_predict flags (fpm_hip.h FPM_PREDICT_*): one kind, optionally | PREDICT_DEVICE
PREDICT_AMPLITUDE, PREDICT_COUNTS, PREDICT_DIFF, PREDICT_DEVICE = 0, 1, 2, 4
PREDICT_KINDS = {"amplitude": PREDICT_AMPLITUDE, "counts": PREDICT_COUNTS, "diff": PREDICT_DIFF}
GRAD_DEVICE = 1             # fpm_gradient: the gradients are device pointers (fpm_hip.h FPM_GRAD_DEVICE)
# fpm_refocus flags (fpm_hip.h FPM_REFOCUS_*)
REFOCUS_DEVICE = 1          # planes is a device pointer on the context's device
REFOCUS_Z_PER_PATCH = 2     # zl is [nz][n_patch]

# fpm_info.fused_kernel: the LED-update kernel of the context (fpm_hip.h FPM_KERNEL_*)
KERNEL_GENERAL, KERNEL_FUSED_NP256, KERNEL_FUSED_NP200, KERNEL_FUSED_SMALL, KERNEL_FUSED_NP256_DIST = 0, 1, 2, 3, 4
KERNEL_FUSED_NP90 = 5
KERNEL_NAMES = {KERNEL_GENERAL: "general_led_step", KERNEL_FUSED_NP256: "k_fused_iteration",
                KERNEL_FUSED_NP200: "k_fused_mr", KERNEL_FUSED_SMALL: "k_fused_small",
                KERNEL_FUSED_NP256_DIST: "k_fused_dist", KERNEL_FUSED_NP90: "k_fused_s90"}

# every symbol include/fpm_hip.h declares
HIP_SYMBOLS = (
    "fpm_create", "fpm_destroy", "fpm_upload_stack", "fpm_upload_stack_device",
    "fpm_init", "fpm_run", "fpm_synchronize", "fpm_download",
    "fpm_download_objcrop_device", "fpm_set_stream", "fpm_get_info",
    "fpm_get_timing", "fpm_runFPM", "fpm_last_error", "fpm_version",
    "fpm_upload_frames", "fpm_download_stack", "fpm_get_info_sized", "fpm_abi_version",
    "fpm_get_clock", "fpm_residual", "fpm_residual_at", "fpm_set_crops", "fpm_get_crops",
    "fpm_set_gains", "fpm_get_gains", "fpm_moments", "fpm_set_state", "fpm_download_state_device",
    "fpm_stitch_tiles", "fpm_stitch", "fpm_predict", "fpm_refocus",
    "fpm_gradient",
)
# test-only entry points (include/fpm_hip_debug.h)
HIP_DEBUG_SYMBOLS = ("fpm_debug_slot_update", "fpm_debug_update_coef", "fpm_debug_set_stall", "fpm_debug_get_plan",
                     "fpm_debug_get_maxima", "fpm_debug_plan_ladder", "fpm_debug_get_ladder", "fpm_debug_objcrop",
                     "fpm_debug_plan_objcrop", "fpm_debug_get_objcrop_plan", "fpm_debug_get_band")
# fpm_ladder_kernel.generation
LADDER_ONE_SEQ, LADDER_TILED, LADDER_WAVE = 0, 1, 2
# fpm_objcrop_plan.kind
OBJCROP_REGS_256M, OBJCROP_REGS_600, OBJCROP_REGS_360, OBJCROP_SIX_STEP_4K, OBJCROP_BATCHED = 0, 1, 2, 3, 4
# fpm_debug_get_plan: general_kind / residual_kind values
GENERAL_REG1024, GENERAL_REG256, GENERAL_LDS = 0, 1, 2
RESIDUAL_REG256, RESIDUAL_LDS = 0, 1
ABI_VERSION = 6  # include/fpm_hip.h FPM_ABI_VERSION this mirror follows


class FpmError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"fpm error {code}: {msg}")
        self.code = code


class fpm_problem(C.Structure):
    _fields_ = [
        ("np", C.c_int32), ("nlarge", C.c_int32), ("n_stack", C.c_int32),
        ("n_order", C.c_int32), ("order", C.POINTER(C.c_int32)),
        ("crop_x0", C.POINTER(C.c_int32)), ("crop_y0", C.POINTER(C.c_int32)),
        ("na_radius", C.c_int32), ("init_pos", C.c_int32),
        ("delta1", C.c_double), ("delta2", C.c_double), ("eps", C.c_double),
        ("n_patch", C.c_int32), ("path", C.c_int32), ("flags", C.c_uint32),
    ]


class fpm_frames(C.Structure):
    _fields_ = [
        ("height", C.c_int32), ("width", C.c_int32),
        ("patch_x0", C.POINTER(C.c_int32)), ("patch_y0", C.POINTER(C.c_int32)),
        ("bk1_x", C.c_int32), ("bk1_y", C.c_int32), ("bk2_x", C.c_int32), ("bk2_y", C.c_int32),
        ("bg_threshold", C.c_double), ("darkfield_exp_multiplier", C.c_double),
        ("darkfield", C.POINTER(C.c_uint8)),
    ]


class fpm_info(C.Structure):
    _fields_ = [("path", C.c_int32), ("box", C.c_int32), ("support_px", C.c_int32),
                ("device", C.c_int32), ("device_bytes", C.c_size_t), ("wg_per_patch", C.c_int32),
                ("fused_kernel", C.c_int32), ("threads_per_wg", C.c_int32)]


class fpm_timing(C.Structure):
    _fields_ = [("run_ms", C.c_double), ("led_ms", C.c_double),
                ("led_launch_ms", C.c_double), ("led_launches", C.c_int32),
                ("objcrop_ms", C.c_double)]


class fpm_clock(C.Structure):
    _fields_ = [("clock_mhz", C.c_double), ("cycles_per_launch", C.c_double),
                ("ms_per_launch", C.c_double), ("launches", C.c_int32)]


class fpm_probe(C.Structure):
    _fields_ = [("pos", C.c_int32), ("dx", C.c_int32), ("dy", C.c_int32)]


class fpm_stitch_grid(C.Structure):
    _fields_ = [("gy", C.c_int32), ("gx", C.c_int32), ("tile", C.c_int32),
                ("stride_y", C.c_int32), ("stride_x", C.c_int32)]


class fpm_ladder_kernel(C.Structure):
    _fields_ = [("generation", C.c_int), ("tile", C.c_int), ("threads", C.c_int), ("e", C.c_int),
                ("grid_x", C.c_int), ("grid_y", C.c_int), ("lds_dynamic", C.c_int), ("lds_static", C.c_int)]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


class fpm_ladder(C.Structure):
    _fields_ = [("rows", fpm_ladder_kernel), ("cols", fpm_ladder_kernel)]

    def as_dict(self):
        return dict(rows=self.rows.as_dict(), cols=self.cols.as_dict())


class fpm_objcrop_plan(C.Structure):
    _fields_ = [("kind", C.c_int), ("per_block", C.c_int), ("rows_lds_dynamic", C.c_int), ("rows_lds_static", C.c_int),
                ("cols_lds_dynamic", C.c_int), ("cols_lds_static", C.c_int)]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


_lib = None


def load_library(path: str = HIP_LIB):
    """Load libfpm_hip.so (raises OSError when it is missing -- no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise OSError(f"{path} not built: run `make -C fpm-opencv_amd` "
                      "(or __graft_entry__.build())")
    lib = C.CDLL(path)
    vp = C.c_void_p
    f32p = C.POINTER(C.c_float)
    u16p = C.POINTER(C.c_uint16)
    sig = {
        "fpm_create": (C.c_int, [C.POINTER(fpm_problem), C.c_int, C.POINTER(vp)]),
        "fpm_destroy": (None, [vp]),
        "fpm_upload_stack": (C.c_int, [vp, u16p]),
        "fpm_upload_stack_device": (C.c_int, [vp, vp]),
        "fpm_init": (C.c_int, [vp]),
        "fpm_run": (C.c_int, [vp, C.c_int]),
        "fpm_synchronize": (C.c_int, [vp]),
        "fpm_download": (C.c_int, [vp, f32p, f32p, f32p, f32p]),
        "fpm_download_objcrop_device": (C.c_int, [vp, vp]),
        "fpm_set_stream": (C.c_int, [vp, vp]),
        "fpm_get_info": (C.c_int, [vp, C.POINTER(fpm_info)]),
        "fpm_get_info_sized": (C.c_int, [vp, C.POINTER(fpm_info), C.c_size_t]),
        "fpm_abi_version": (C.c_int, []),
        "fpm_debug_set_stall": (C.c_int, [vp, C.c_int]),
        "fpm_debug_get_plan": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "fpm_debug_get_maxima": (C.c_int, [vp, C.POINTER(C.c_int), f32p, C.POINTER(C.c_uint8), f32p, f32p]),
        "fpm_debug_get_band": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "fpm_debug_plan_ladder": (C.c_int, [C.c_int] * 6 + [C.POINTER(fpm_ladder)]),
        "fpm_debug_get_ladder": (C.c_int, [vp, C.c_int, C.POINTER(fpm_ladder)]),
        "fpm_debug_objcrop": (C.c_int, [vp, f32p, C.POINTER(C.c_int), f32p]),
        "fpm_debug_plan_objcrop": (C.c_int, [C.c_int] * 3 + [C.POINTER(fpm_objcrop_plan)]),
        "fpm_debug_get_objcrop_plan": (C.c_int, [vp, C.POINTER(fpm_objcrop_plan)]),
        "fpm_get_timing": (C.c_int, [vp, C.POINTER(fpm_timing)]),
        "fpm_get_clock": (C.c_int, [vp, C.POINTER(fpm_clock)]),
        "fpm_residual": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "fpm_residual_at": (C.c_int, [vp, C.POINTER(fpm_probe), C.c_int, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "fpm_set_crops": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "fpm_get_crops": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "fpm_set_gains": (C.c_int, [vp, f32p]),
        "fpm_get_gains": (C.c_int, [vp, f32p]),
        "fpm_moments": (C.c_int, [vp, C.POINTER(fpm_probe), C.c_int] + [C.POINTER(C.c_double)] * 4),
        "fpm_predict": (C.c_int, [vp, C.POINTER(fpm_probe), C.c_int, C.c_uint32, vp, C.POINTER(C.c_double)]),
        "fpm_gradient": (C.c_int, [vp, C.POINTER(fpm_probe), C.c_int, C.c_uint32, vp, vp] + [C.POINTER(C.c_double)] * 3),
        "fpm_refocus": (C.c_int, [vp, C.POINTER(C.c_double), C.c_int, C.c_double, C.c_int, C.c_uint32, vp]
                        + [C.POINTER(C.c_double)] * 4),
        "fpm_set_state": (C.c_int, [vp, vp, vp, C.c_uint32]),
        "fpm_download_state_device": (C.c_int, [vp, vp, vp]),
        "fpm_stitch_tiles": (C.c_int, [C.c_int, vp, C.POINTER(fpm_stitch_grid), C.c_uint32, vp,
                                       C.POINTER(C.c_double), vp, C.POINTER(C.c_double)]),
        "fpm_stitch": (C.c_int, [vp, C.POINTER(fpm_stitch_grid), C.c_uint32, vp, C.POINTER(C.c_double),
                                 C.POINTER(C.c_double)]),
        "fpm_runFPM": (C.c_int, [C.POINTER(fpm_problem), C.c_int, u16p, C.c_int,
                                 f32p, f32p, f32p, f32p]),
        "fpm_upload_frames": (C.c_int, [vp, C.POINTER(fpm_frames), vp, C.c_int, C.POINTER(C.c_int16)]),
        "fpm_download_stack": (C.c_int, [vp, u16p]),
        "fpm_last_error": (C.c_char_p, []),
        "fpm_version": (C.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.fpm_abi_version() != ABI_VERSION:
        raise OSError(f"{path}: ABI {lib.fpm_abi_version()}, this mirror follows ABI {ABI_VERSION}: rebuild")
    _lib = lib
    return lib


def _check(rc: int):
    if rc != FPM_OK:
        raise FpmError(rc, _lib.fpm_last_error().decode())


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _f32p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


@dataclass
class Problem:
    """Flattened ``FPM_Dataset`` fields runFPM reads."""
    np_: int
    L: int
    order: np.ndarray
    x0: np.ndarray
    y0: np.ndarray
    radius: int
    delta1: float
    delta2: float
    n_patch: int = 1
    init_pos: int = 1
    eps: float = float(np.float32(1e-10))
    path: int = PATH_AUTO
    flags: int = 0
    _keep: list = field(default_factory=list, repr=False)

    def to_c(self) -> fpm_problem:
        order, x0, y0 = _i32(self.order), _i32(self.x0), _i32(self.y0)
        self._keep[:] = [order, x0, y0]
        p = fpm_problem()
        p.np = self.np_
        p.nlarge = self.L
        p.n_stack = len(x0)
        p.n_order = len(order)
        p.order = order.ctypes.data_as(C.POINTER(C.c_int32))
        p.crop_x0 = x0.ctypes.data_as(C.POINTER(C.c_int32))
        p.crop_y0 = y0.ctypes.data_as(C.POINTER(C.c_int32))
        p.na_radius = self.radius
        p.init_pos = self.init_pos
        p.delta1 = float(self.delta1)
        p.delta2 = float(self.delta2)
        p.eps = float(self.eps)
        p.n_patch = self.n_patch
        p.path = self.path
        p.flags = self.flags
        return p


class Solver:
    """One fpm_ctx on one GPU."""

    def __init__(self, prob: Problem, device: int = 0):
        lib = load_library()
        self.prob = prob
        self._cprob = prob.to_c()
        h = C.c_void_p()
        _check(lib.fpm_create(C.byref(self._cprob), device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.fpm_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def upload(self, stack: np.ndarray):
        """stack: uint16 [n_stack][n_patch][Np][Np] (or [n_stack][Np][Np] if n_patch == 1)."""
        p = self.prob
        a = np.ascontiguousarray(stack, dtype=np.uint16)
        want = (len(p.x0), p.n_patch, p.np_, p.np_)
        if a.ndim == 3 and p.n_patch == 1:
            a = a[:, None]
        if a.shape != want:
            raise ValueError(f"stack shape {a.shape} != {want}")
        _check(_lib.fpm_upload_stack(self._h, a.ctypes.data_as(C.POINTER(C.c_uint16))))

    def upload_frames(self, frames, patch_x0, patch_y0, bk1=(1, 1), bk2=(1, 1), bg_threshold=1000.0,
                      darkfield_exp_multiplier=1.0, darkfield=None, device_ptr: int | None = None,
                      shape=None):
        """Loader preprocessing on the GPU (fpmMain.cpp:124-144): `frames` is
        uint16 [n_stack][H][W] on the host, or pass device_ptr (+ shape=(H, W))
        for frames already in device memory.  Returns the int16 bg_val per image."""
        p = self.prob
        n = len(p.x0)
        if device_ptr is None:
            a = np.ascontiguousarray(frames, dtype=np.uint16)
            if a.ndim != 3 or a.shape[0] != n:
                raise ValueError(f"frames shape {a.shape}: want [{n}][H][W]")
            H, W = a.shape[1:]
            data = a.ctypes.data_as(C.c_void_p)
        else:
            H, W = shape
            data = C.c_void_p(device_ptr)
        px, py = _i32(patch_x0), _i32(patch_y0)
        if len(px) != p.n_patch or len(py) != p.n_patch:
            raise ValueError("one (x0, y0) per patch")
        dark = np.ascontiguousarray(np.zeros(n, np.uint8) if darkfield is None else np.asarray(darkfield, np.uint8))
        f = fpm_frames(int(H), int(W), px.ctypes.data_as(C.POINTER(C.c_int32)), py.ctypes.data_as(C.POINTER(C.c_int32)),
                       int(bk1[0]), int(bk1[1]), int(bk2[0]), int(bk2[1]), float(bg_threshold),
                       float(darkfield_exp_multiplier), dark.ctypes.data_as(C.POINTER(C.c_uint8)))
        bg = np.zeros(n, np.int16)
        _check(_lib.fpm_upload_frames(self._h, C.byref(f), data, 0 if device_ptr is None else 1,
                                      bg.ctypes.data_as(C.POINTER(C.c_int16))))
        return bg

    def download_stack(self) -> np.ndarray:
        p = self.prob
        out = np.empty((len(p.x0), p.n_patch, p.np_, p.np_), np.uint16)
        _check(_lib.fpm_download_stack(self._h, out.ctypes.data_as(C.POINTER(C.c_uint16))))
        return out

    def upload_device(self, ptr: int):
        _check(_lib.fpm_upload_stack_device(self._h, C.c_void_p(ptr)))

    def set_stream(self, stream_ptr: int | None):
        _check(_lib.fpm_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    def init(self):
        _check(_lib.fpm_init(self._h))

    def run(self, iters: int):
        _check(_lib.fpm_run(self._h, int(iters)))

    def synchronize(self):
        _check(_lib.fpm_synchronize(self._h))

    def residual(self):
        """Data-fidelity residual of the current state (fpm_residual; read-only,
        blocking): err[i][b] = sum (|psi| - g sqrt(I))^2 (g: gains()) and ref[i][b] = sum I for
        the LED at order[i] and patch b, float64 [n_order][n_patch], and the
        sweep's event time ms."""
        p = self.prob
        err = np.empty((len(p.order), p.n_patch), np.float64)
        ref = np.empty_like(err)
        ms = C.c_double()
        dp = C.POINTER(C.c_double)
        _check(_lib.fpm_residual(self._h, err.ctypes.data_as(dp), ref.ctypes.data_as(dp), C.byref(ms)))
        return dict(err=err, ref=ref, ms=ms.value)

    @staticmethod
    def _probes(pos, dx, dy):
        pos, dx, dy = _i32(pos).ravel(), _i32(dx).ravel(), _i32(dy).ravel()
        if not (len(pos) == len(dx) == len(dy)):
            raise ValueError("pos, dx and dy must have one length")
        n = len(pos)
        probes = (fpm_probe * max(n, 1))()
        for k in range(n):
            probes[k] = fpm_probe(int(pos[k]), int(dx[k]), int(dy[k]))
        return probes, n

    def residual_at(self, pos, dx, dy):
        """fpm_residual_at: the residual of the current state for the image of
        order[pos[k]] with its window moved by (dx[k], dy[k]) from the crop
        table's; equal-length integer arrays.  err / ref are float64
        [n][n_patch], row k = entry k; read-only, blocking."""
        probes, n = self._probes(pos, dx, dy)
        err = np.empty((n, self.prob.n_patch), np.float64)
        ref = np.empty_like(err)
        ms = C.c_double()
        dp = C.POINTER(C.c_double)
        _check(_lib.fpm_residual_at(self._h, probes, n, err.ctypes.data_as(dp), ref.ctypes.data_as(dp), C.byref(ms)))
        return dict(err=err, ref=ref, ms=ms.value)

    def moments(self, pos=None, dx=None, dy=None):
        """fpm_moments: the raw sums a gain is estimated from, of the current
        state: model Q = sum |psi|^2, cross C = sum |psi| sqrt(I), ref S = sum I,
        float64 [n][n_patch], and the sweep's event time ms.  Without arguments
        the rows are the positions of order[] (as residual()); with pos / dx / dy
        they are residual_at's entries.  The gain table does not enter:
        E(g) = Q - 2 g C + g^2 S.  Read-only, blocking."""
        if pos is None:
            if dx is not None or dy is not None:
                raise ValueError("dx / dy without pos")
            probes, n = None, len(self.prob.order)
        else:
            probes, n = self._probes(pos, np.zeros_like(_i32(pos)) if dx is None else dx,
                                     np.zeros_like(_i32(pos)) if dy is None else dy)
        out = [np.empty((n, self.prob.n_patch), np.float64) for _ in range(3)]
        ms = C.c_double()
        dp = C.POINTER(C.c_double)
        _check(_lib.fpm_moments(self._h, probes, n, *(a.ctypes.data_as(dp) for a in out), C.byref(ms)))
        return dict(model=out[0], cross=out[1], ref=out[2], ms=ms.value)

    def predict(self, kind: str = "amplitude", pos=None, dx=None, dy=None, device_ptr: int | None = None):
        """fpm_predict: the forward model's images of the current state,
        [n][n_patch][Np][Np] with pixel (y, x) at [y][x].  kind "amplitude":
        float32 |psi| (the gains do not enter); "counts": uint16
        rint((|psi| / g)^2) saturated at 65535, what the camera would record;
        "diff": float32 |psi| - g sqrt(I) (needs the stack).  Without pos the
        rows are the positions of order[]; with pos / dx / dy they are
        residual_at's entries.  Returns the array, or None when device_ptr
        names device memory of the caller's that receives it.  The kernels'
        event time is left in predict_ms.  Read-only, blocking."""
        if kind not in PREDICT_KINDS:
            raise ValueError(f"kind {kind!r}: want one of {sorted(PREDICT_KINDS)}")
        flags = PREDICT_KINDS[kind]
        if pos is None:
            if dx is not None or dy is not None:
                raise ValueError("dx / dy without pos")
            probes, n = None, len(self.prob.order)
        else:
            probes, n = self._probes(pos, np.zeros_like(_i32(pos)) if dx is None else dx,
                                     np.zeros_like(_i32(pos)) if dy is None else dy)
        out = None
        if device_ptr is None:
            p = self.prob
            out = np.empty((n, p.n_patch, p.np_, p.np_), np.uint16 if kind == "counts" else np.float32)
            dst = out.ctypes.data_as(C.c_void_p)
        else:
            dst, flags = C.c_void_p(device_ptr), flags | PREDICT_DEVICE
        ms = C.c_double()
        _check(_lib.fpm_predict(self._h, probes, n, flags, dst, C.byref(ms)))
        self.predict_ms = ms.value
        return out

    def gradient(self, pos=None, dx=None, dy=None, objF: bool = True, pupil: bool = True, sums: bool = False,
                 device_ptrs=None):
        """fpm_gradient: G = df/dRe + i df/dIm of the data-fidelity cost
        f = sum E (residual()'s err, gains included) of the current state, so
        that df = sum Re(conj(G) dz): PyTorch's convention, twice df/dconj(z).
        Without pos the list is order[]; with pos / dx / dy it is residual_at's
        entries (an LED may repeat; each entry counts once).  Returns a dict:
        objF complex64 [n_patch][L][L] un-centred and pupil complex64
        [n_patch][Np][Np] centred (download()'s layouts; exactly zero outside
        the entries' disks / the support), each present when asked for; with
        sums, err / ref float64 [n][n_patch] of the same pass.  device_ptrs =
        (objF_ptr, pupil_ptr), either None / 0: device memory of the caller's
        (float32 pairs) receives the gradients instead and the dict holds only
        the sums.  The kernels' event time is left in gradient_ms.  Read-only,
        blocking."""
        p = self.prob
        if pos is None:
            if dx is not None or dy is not None:
                raise ValueError("dx / dy without pos")
            probes, n = None, len(p.order)
        else:
            probes, n = self._probes(pos, np.zeros_like(_i32(pos)) if dx is None else dx,
                                     np.zeros_like(_i32(pos)) if dy is None else dy)
        out, flags = {}, 0
        if device_ptrs is not None:
            po, pp = (C.c_void_p(q or 0) for q in device_ptrs)
            flags = GRAD_DEVICE
        else:
            if objF:
                out["objF"] = np.empty((p.n_patch, p.L, p.L), np.complex64)
            if pupil:
                out["pupil"] = np.empty((p.n_patch, p.np_, p.np_), np.complex64)
            po, pp = (out[k].ctypes.data_as(C.c_void_p) if k in out else None for k in ("objF", "pupil"))
        dp = C.POINTER(C.c_double)
        if sums:
            out["err"] = np.empty((n, p.n_patch), np.float64)
            out["ref"] = np.empty_like(out["err"])
        ms = C.c_double()
        _check(_lib.fpm_gradient(self._h, probes, n, flags, po, pp, out["err"].ctypes.data_as(dp) if sums else None,
                                 out["ref"].ctypes.data_as(dp) if sums else None, C.byref(ms)))
        self.gradient_ms = ms.value
        return out

    def refocus(self, zl, fl: float, margin: int = 0, planes: bool = True, device_ptr: int | None = None,
                sums: bool = True):
        """fpm_refocus: the field of the current state propagated to the planes
        zl = z / lambda (1-D [nz]: one z for every patch; 2-D [nz][n_patch]: a z
        per patch) by the angular-spectrum method, fl = lambda / (L ps) the
        normalised frequency of one spectrum bin (focus.bin_frequency).  Returns
        (planes, sums): planes complex64 [nz][n_patch][L][L], or None when
        planes is False (the autofocus sweep: nothing but the sums leaves the
        device) or device_ptr names device memory of the caller's that receives
        them; sums = dict(sum_a, sum_a2, sum_g), float64 [nz][n_patch] over the
        interior [margin, L - margin)^2 (focus.measures makes the focus measures
        of them), or None when sums is False.  The kernels' event time is left
        in refocus_ms.  Read-only, blocking."""
        p = self.prob
        z = np.ascontiguousarray(zl, dtype=np.float64)
        flags = 0
        if z.ndim == 2:
            if z.shape[1] != p.n_patch:
                raise ValueError(f"zl shape {z.shape}: want [nz][{p.n_patch}]")
            flags |= REFOCUS_Z_PER_PATCH
        elif z.ndim != 1:
            raise ValueError(f"zl shape {z.shape}: want [nz] or [nz][n_patch]")
        nz = z.shape[0]
        out, dst = None, None
        if device_ptr is not None:
            dst, flags = C.c_void_p(device_ptr), flags | REFOCUS_DEVICE
        elif planes:
            out = np.empty((nz, p.n_patch, p.L, p.L), np.complex64)
            dst = out.ctypes.data_as(C.c_void_p)
        dp = C.POINTER(C.c_double)
        s = [np.empty((nz, p.n_patch), np.float64) for _ in range(3)] if sums else None
        ms = C.c_double()
        _check(_lib.fpm_refocus(self._h, z.ctypes.data_as(dp), nz, float(fl), int(margin), flags, dst,
                                *((a.ctypes.data_as(dp) for a in s) if sums else (None, None, None)), C.byref(ms)))
        self.refocus_ms = ms.value
        return out, (dict(sum_a=s[0], sum_a2=s[1], sum_g=s[2]) if sums else None)

    def set_gains(self, g):
        """fpm_set_gains: the per-image amplitude factor, float32
        [n_stack][n_patch] ([n_stack] if n_patch == 1); None = all ones.  Every
        value finite and > 0.  The state is kept."""
        if g is None:
            _check(_lib.fpm_set_gains(self._h, None))
            return
        want = (len(self.prob.x0), self.prob.n_patch)
        a = np.ascontiguousarray(g, dtype=np.float32)
        if a.ndim == 1 and want[1] == 1:
            a = a[:, None]
        if a.shape != want:
            raise ValueError(f"gain shape {a.shape} != {want}")
        _check(_lib.fpm_set_gains(self._h, _f32p(a)))

    def gains(self) -> np.ndarray:
        """float32 [n_stack][n_patch]: the gain table in use (fpm_get_gains)."""
        g = np.empty((len(self.prob.x0), self.prob.n_patch), np.float32)
        _check(_lib.fpm_get_gains(self._h, _f32p(g)))
        return g

    def set_crops(self, x0, y0):
        """fpm_set_crops: replace the crop table [n_stack] of the live context;
        the state is kept.  Raises FpmError (and changes nothing) when the
        table is invalid or plans another context than this one."""
        x0, y0 = _i32(x0).ravel(), _i32(y0).ravel()
        n = len(self.prob.x0)
        if len(x0) != n or len(y0) != n:
            raise ValueError(f"crop tables of {len(x0)} / {len(y0)} entries: want {n}")
        ip = C.POINTER(C.c_int32)
        _check(_lib.fpm_set_crops(self._h, x0.ctypes.data_as(ip), y0.ctypes.data_as(ip)))

    def crops(self):
        """(x0, y0) int32 [n_stack]: the crop table in use (fpm_get_crops)."""
        n = len(self.prob.x0)
        x0, y0 = np.empty(n, np.int32), np.empty(n, np.int32)
        ip = C.POINTER(C.c_int32)
        _check(_lib.fpm_get_crops(self._h, x0.ctypes.data_as(ip), y0.ctypes.data_as(ip)))
        return x0, y0

    def download(self, objF=True, objCrop=True, pupil=True, support=True):
        p = self.prob
        B, L, N = p.n_patch, p.L, p.np_
        oF = np.empty((B, L, L), np.complex64) if objF else None
        oC = np.empty((B, L, L), np.complex64) if objCrop else None
        pu = np.empty((B, N, N), np.complex64) if pupil else None
        su = np.empty((B, N, N), np.float32) if support else None
        _check(_lib.fpm_download(self._h, _f32p(oF), _f32p(oC), _f32p(pu), _f32p(su)))
        return dict(objF=oF, objCrop=oC, pupil=pu, support=su)

    def _pairs(self, a, want, name):
        """complex64, or float32 with a trailing axis of 2 (re, im), as a contiguous complex64 of shape `want`."""
        a = np.asarray(a)
        if a.dtype == np.float32 and a.ndim == len(want) + 1 and a.shape[-1] == 2:
            a = np.ascontiguousarray(a).view(np.complex64)[..., 0]
        elif a.dtype != np.complex64:
            raise ValueError(f"{name}: dtype {a.dtype}, want complex64 or float32 (re, im) pairs")
        if a.shape != want:
            raise ValueError(f"{name} shape {a.shape} != {want}")
        return np.ascontiguousarray(a)

    def set_state(self, objF=None, pupil=None):
        """fpm_set_state from host arrays in download()'s layouts: objF
        [n_patch][L][L] un-centred ([L][L] if n_patch == 1), pupil
        [n_patch][Np][Np] centred, or 2-D [Np][Np] = one pupil for every patch;
        complex64 or float32 pairs.  None keeps what the context has (not
        both).  With both given it replaces init().  Raises FpmError, the
        context unchanged, when a value is not finite, the spectrum is nonzero
        outside the live band or the pupil vanishes on the support."""
        p = self.prob
        flags = 0
        if objF is not None:
            o = np.asarray(objF)
            if p.n_patch == 1 and o.ndim == (3 if o.dtype == np.float32 else 2):
                o = o[None]
            objF = self._pairs(o, (p.n_patch, p.L, p.L), "objF")
        if pupil is not None:
            q = np.asarray(pupil)
            if q.ndim == (3 if q.dtype == np.float32 else 2):
                flags |= STATE_PUPIL_SHARED
                pupil = self._pairs(q, (p.np_, p.np_), "pupil")
            else:
                pupil = self._pairs(q, (p.n_patch, p.np_, p.np_), "pupil")
        _check(_lib.fpm_set_state(self._h, None if objF is None else objF.ctypes.data_as(C.c_void_p),
                                  None if pupil is None else pupil.ctypes.data_as(C.c_void_p), flags))

    def set_state_device(self, objF_ptr: int | None, pupil_ptr: int | None, pupil_shared: bool = False):
        """fpm_set_state from device memory on the context's device (float32
        pairs in set_state's layouts); a pointer of None / 0 keeps what the
        context has."""
        _check(_lib.fpm_set_state(self._h, C.c_void_p(objF_ptr or 0), C.c_void_p(pupil_ptr or 0),
                                  STATE_DEVICE | (STATE_PUPIL_SHARED if pupil_shared else 0)))

    def download_state_device(self, objF_ptr: int | None, pupil_ptr: int | None):
        """fpm_download_state_device: the un-centred fp32 spectrum
        [n_patch][L][L][2] and the centred pupil [n_patch][Np][Np][2] into
        device memory of the caller's; None / 0 skips one."""
        _check(_lib.fpm_download_state_device(self._h, C.c_void_p(objF_ptr or 0), C.c_void_p(pupil_ptr or 0)))

    def stitch(self, grid, stride, align: str = "none", device_ptr: int | None = None):
        """fpm_stitch: the context's objCrop tiles (n_patch == gy * gx, row-major)
        at strides `stride` (one int, or (stride_y, stride_x), in high-resolution
        pixels, ceil(L/2) .. L) aligned ("none" | "phase" | "complex") and
        blended into one field.  Returns (field, factors): field complex64
        [H][W] (stitch_shape), or None when device_ptr names device memory of
        the caller's that receives it; factors complex128 [n_patch].  Read-only
        on the context, blocking."""
        g = _stitch_grid(grid, self.prob.L, stride)
        flags = _stitch_flags(align)
        field = None
        if device_ptr is None:
            field = np.empty(tuple(max(v, 0) for v in stitch_shape(grid, self.prob.L, stride)), np.complex64)
            dst = field.ctypes.data_as(C.c_void_p)
        else:
            dst, flags = C.c_void_p(device_ptr), flags | STITCH_DEVICE
        fac = np.empty(max(g.gy * g.gx, 1), np.complex128)
        _check(_lib.fpm_stitch(self._h, C.byref(g), flags, dst, fac.ctypes.data_as(C.POINTER(C.c_double)), None))
        return field, fac

    def download_objcrop_device(self, ptr: int):
        _check(_lib.fpm_download_objcrop_device(self._h, C.c_void_p(ptr)))

    def info(self) -> fpm_info:
        i = fpm_info()
        _check(_lib.fpm_get_info_sized(self._h, C.byref(i), C.sizeof(i)))
        return i

    def debug_set_stall(self, led: int):
        """Test-only fault injection (include/fpm_hip_debug.h): from LED
        position `led` on, the last workgroup of each patch stops publishing
        its split / distributed-mode handoffs; -1 switches it off."""
        _check(_lib.fpm_debug_set_stall(self._h, int(led)))

    def debug_plan(self) -> dict:
        """Test-only (include/fpm_hip_debug.h): the stack's device layout meas_g,
        the general path's kind (GENERAL_*, -1 fused) and the residual sweep's
        kernel pair (RESIDUAL_*)."""
        g, k, r = C.c_int(), C.c_int(), C.c_int()
        _check(_lib.fpm_debug_get_plan(self._h, C.byref(g), C.byref(k), C.byref(r)))
        return dict(meas_g=g.value, general_kind=k.value, residual_kind=r.value)

    def debug_band(self) -> tuple:
        """Test-only (include/fpm_hip_debug.h): the live band (sy0, sy1, sx0, sx1),
        inclusive, of the centred spectrum: set_state() refuses a spectrum that
        is nonzero outside it."""
        band = (C.c_int * 4)()
        _check(_lib.fpm_debug_get_band(self._h, band))
        return tuple(int(v) for v in band)

    def debug_maxima(self) -> dict:
        """Test-only (include/fpm_hip_debug.h): the carried max|objF| / max|P|
        bookkeeping after synchronising the stream, in full tile coordinates of
        the centred spectrum: tmax float32 [B][nty][ntx], dirty bool
        [B][nty][ntx], rmax float32 [B][nty] (None on a fused context), pmax
        float32 [B][npart].  Read-only."""
        dims = (C.c_int * 4)()
        _check(_lib.fpm_debug_get_maxima(self._h, dims, None, None, None, None))
        nty, ntx, npart, has_rmax = (int(v) for v in dims)
        B = self.prob.n_patch
        tmax = np.empty((B, nty, ntx), np.float32)
        dirty = np.empty((B, nty, ntx), np.uint8)
        rmax = np.empty((B, nty), np.float32) if has_rmax else None
        pmax = np.empty((B, npart), np.float32)
        _check(_lib.fpm_debug_get_maxima(self._h, dims, _f32p(tmax), dirty.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         _f32p(rmax), _f32p(pmax)))
        return dict(tmax=tmax, dirty=dirty.astype(bool), rmax=rmax, pmax=pmax)

    def debug_ladder(self, residual: bool = False) -> dict:
        """Test-only (include/fpm_hip_debug.h): the rung of the LDS kernel ladder
        the context's update step (or, residual=True, its sweep) launches, as
        debug_plan_ladder returns it."""
        l = fpm_ladder()
        _check(_lib.fpm_debug_get_ladder(self._h, int(residual), C.byref(l)))
        return l.as_dict()

    def debug_objcrop_plan(self) -> dict:
        """Test-only (include/fpm_hip_debug.h): what the context's objCrop
        launches, as debug_plan_objcrop returns it."""
        o = fpm_objcrop_plan()
        _check(_lib.fpm_debug_get_objcrop_plan(self._h, C.byref(o)))
        return o.as_dict()

    def debug_objcrop(self, spec, band) -> np.ndarray:
        """Test-only (include/fpm_hip_debug.h): objCrop of the CENTRED spectrum
        `spec`, complex64 [n_patch][L][L], with the live band (sy0, sy1, sx0, sx1)
        inclusive, through the context's own objCrop launch; complex64
        [n_patch][L][L].  The context's state is gone afterwards: init() again
        before run() or download()."""
        p = self.prob
        a = np.ascontiguousarray(spec, dtype=np.complex64)
        want = (p.n_patch, p.L, p.L)
        if a.shape != want:
            raise ValueError(f"spectrum shape {a.shape} != {want}")
        if len(band) != 4:
            raise ValueError("band is (sy0, sy1, sx0, sx1)")
        out = np.empty(want, np.complex64)
        _check(_lib.fpm_debug_objcrop(self._h, _f32p(a), (C.c_int * 4)(*(int(v) for v in band)), _f32p(out)))
        return out

    def timing(self) -> fpm_timing:
        t = fpm_timing()
        _check(_lib.fpm_get_timing(self._h, C.byref(t)))
        return t

    def clock(self) -> fpm_clock:
        """Shader clock and cycles of the last run's LED-update launches
        (fused path; launches == 0 on the general path)."""
        k = fpm_clock()
        _check(_lib.fpm_get_clock(self._h, C.byref(k)))
        return k


def debug_plan_ladder(np_: int, nb: int, B: int, step: bool = True, no_wave_cols: bool = False,
                      one_seq: bool = False) -> dict:
    """Test-only (include/fpm_hip_debug.h): what the general path's planner
    picks for (Np, nb, B): {"rows": ..., "cols": ...}, each with generation
    (LADDER_*), tile, threads, e, grid_x, grid_y, lds_dynamic, lds_static.
    Needs no GPU."""
    lib = load_library()
    l = fpm_ladder()
    _check(lib.fpm_debug_plan_ladder(int(np_), int(nb), int(B), int(step), int(no_wave_cols), int(one_seq),
                                     C.byref(l)))
    return l.as_dict()


def debug_plan_objcrop(L: int, fp16: bool = False, no_crop4k: bool = False) -> dict:
    """Test-only (include/fpm_hip_debug.h): what the objCrop planner picks for
    Nlarge = L: kind (OBJCROP_*), per_block, and the dynamic / static LDS bytes
    of the row and column launches.  Needs no GPU."""
    lib = load_library()
    o = fpm_objcrop_plan()
    _check(lib.fpm_debug_plan_objcrop(int(L), int(fp16), int(no_crop4k), C.byref(o)))
    return o.as_dict()


def _stitch_strides(stride):
    sy, sx = (stride, stride) if np.ndim(stride) == 0 else stride
    return int(sy), int(sx)


def _stitch_grid(grid, L, stride) -> fpm_stitch_grid:
    gy, gx = grid
    sy, sx = _stitch_strides(stride)
    return fpm_stitch_grid(int(gy), int(gx), int(L), sy, sx)


def _stitch_flags(align: str) -> int:
    if align not in STITCH_ALIGN:
        raise ValueError(f"align {align!r}: one of {sorted(STITCH_ALIGN)}")
    return STITCH_ALIGN[align]


def stitch_shape(grid, L: int, stride) -> tuple:
    """(H, W) of the field of a (gy, gx) grid of L x L tiles at strides `stride`."""
    sy, sx = _stitch_strides(stride)
    return (int(grid[0]) - 1) * sy + int(L), (int(grid[1]) - 1) * sx + int(L)


def stitch_tiles_device(tiles_ptr: int, field_ptr: int, grid, L: int, stride, align: str = "none", device: int = 0,
                        stream_ptr: int | None = None):
    """fpm_stitch_tiles with FPM_STITCH_DEVICE: tiles [gy*gx][L][L] and field
    [H][W] (stitch_shape), float32 pairs, in device memory on `device`; the
    tiles are read in place.  Returns (factors complex128 [gy*gx], the kernels'
    event time in ms).  Blocking."""
    lib = load_library()
    g = _stitch_grid(grid, L, stride)
    fac = np.empty(max(g.gy * g.gx, 1), np.complex128)
    ms = C.c_double()
    _check(lib.fpm_stitch_tiles(int(device), C.c_void_p(tiles_ptr or 0), C.byref(g), _stitch_flags(align) | STITCH_DEVICE,
                                C.c_void_p(field_ptr or 0), fac.ctypes.data_as(C.POINTER(C.c_double)),
                                C.c_void_p(stream_ptr or 0), C.byref(ms)))
    return fac, ms.value


def stitch_tiles(tiles, grid, stride, align: str = "none", device: int = 0):
    """fpm_stitch_tiles on host arrays: tiles complex64 [gy*gx][L][L] (or
    float32 with a trailing axis of 2), tile t = i*gx + j at rows i*stride_y,
    columns j*stride_x.  Returns (field complex64 [H][W], factors complex128
    [gy*gx]).  Blocking; the GPU does the work (device scratch of the call)."""
    lib = load_library()
    a = np.asarray(tiles)
    if a.dtype == np.float32 and a.ndim == 4 and a.shape[-1] == 2:
        a = np.ascontiguousarray(a).view(np.complex64)[..., 0]
    if a.dtype != np.complex64 or a.ndim != 3 or a.shape[1] != a.shape[2]:
        raise ValueError(f"tiles {a.dtype} {a.shape}: want complex64 [P][L][L]")
    a = np.ascontiguousarray(a)
    if a.shape[0] != int(grid[0]) * int(grid[1]):
        raise ValueError(f"{a.shape[0]} tiles for a {grid[0]}x{grid[1]} grid")
    L = a.shape[1]
    g = _stitch_grid(grid, L, stride)
    flags = _stitch_flags(align)
    H, W = stitch_shape(grid, L, stride)
    field = np.empty((max(H, 0), max(W, 0)), np.complex64)
    fac = np.empty(a.shape[0], np.complex128)
    _check(lib.fpm_stitch_tiles(int(device), a.ctypes.data_as(C.c_void_p), C.byref(g), flags,
                                field.ctypes.data_as(C.c_void_p), fac.ctypes.data_as(C.POINTER(C.c_double)),
                                None, None))
    return field, fac


def normalised_residual(d) -> np.ndarray:
    """Per-patch normalised residual sum_i E / sum_i S of a Solver.residual() dict."""
    return np.asarray(d["err"], np.float64).sum(0) / np.asarray(d["ref"], np.float64).sum(0)


def scatter_to_stack(prob: Problem, rows: np.ndarray) -> np.ndarray:
    """Rows by position of order[] ([n_order][n_patch][Np][Np], what
    Solver.predict() returns without pos) as a stack [n_stack][n_patch][Np][Np]
    in upload()'s layout; stack indices not in order[] are zero."""
    stack = np.zeros((len(prob.x0),) + rows.shape[1:], rows.dtype)
    stack[np.asarray(prob.order)] = rows
    return stack


def simulate(prob: Problem, objF, pupil, gains=None, device: int = 0) -> np.ndarray:
    """The uint16 stack [n_stack][n_patch][Np][Np] a camera would record of a
    known object spectrum and pupil (set_state's layouts) under the LED gains
    (set_gains' layout; None = all ones): set_state, predict("counts") for
    every position of order[], scattered to the stack indices.  Images of
    stack indices order[] does not name are zero."""
    with Solver(prob, device) as s:
        s.set_state(objF, pupil)
        if gains is not None:
            s.set_gains(gains)
        return scatter_to_stack(prob, s.predict("counts"))


def run_fpm(prob: Problem, stack: np.ndarray, iters: int, device: int = 0):
    """One-shot runFPM equivalent (create, upload, init, run, download)."""
    with Solver(prob, device) as s:
        s.upload(stack)
        s.init()
        s.run(iters)
        return s.download()
