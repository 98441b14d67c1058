"""Filter operations on single images.

* torch CUDA (ROCm) uint8 tensors run on the HIP kernels (csrc/hip/*.hip) on
  torch's current stream;
* numpy arrays / CPU tensors run on the threaded host executor
  (csrc/core/cpu_exec.cpp, bit-identical to the C++ golden path).

Images are HxW (gray) or HxWx3 (RGB, PPM channel order) uint8; a batch of
frames is BxHxWxC (C = 1 or 3) and runs frame by frame through one cached
engine (same kernels, no per-frame setup).  A chain is a
comma-separated filter list, e.g. "gray:ref,contrast:3.5,emboss3" (see
`FILTERS`); consecutive pointwise ops are fused into the neighbouring stencil
kernel.  Reference kernels: grayscaleKernel / contrastKernel / embossKernel
(kernel.cu:31-94) and the OpenCV CPU chain (kern.cpp:58-77).
"""
from __future__ import annotations

import collections
import threading

import numpy as np

from .._native import C

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

# syntax -> one-line description of every chain token: the parser's own table (csrc/core/filters.cpp)
FILTERS = dict(C.filter_catalogue())

_cache_lock = threading.Lock()
_engines: "collections.OrderedDict" = collections.OrderedDict()
_MAX_ENGINES = 8


def _is_tensor(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


def _shape(x):
    if x.ndim == 2:
        return x.shape[1], x.shape[0], 1
    if x.ndim == 3 and x.shape[2] in (1, 3):
        return x.shape[1], x.shape[0], x.shape[2]
    raise ValueError(f"image must be HxW or HxWx3 uint8, got shape {tuple(x.shape)}")


def _engine(W, H, Cc, chain, border, fuse, device_index, halo=True, held=False):
    key = (W, H, Cc, chain, border, fuse, device_index, halo, held)
    with _cache_lock:
        eng = _engines.get(key)
        if eng is not None:
            _engines.move_to_end(key)
            return eng
        cfg = C.EngineConfig()
        cfg.W, cfg.H, cfg.C = int(W), int(H), int(Cc)
        cfg.chain = chain
        cfg.border = C.parse_border(border)
        cfg.fuse = bool(fuse)
        cfg.halo = bool(halo)
        cfg.held_input = bool(held)
        cfg.device = int(device_index)
        cfg.backend = C.Backend.device
        eng = C.Engine(cfg)
        eng._stream = None
        # one call at a time per engine: the C++ calls release the GIL and the
        # engine's ping-pong buffers are shared by every call with this key
        eng._lock = threading.Lock()
        _engines[key] = eng
        while len(_engines) > _MAX_ENGINES:
            _engines.popitem(last=False)
        return eng


def apply(image, chain: str, border: str = "reflect101", fuse: bool = True):
    """Apply a filter chain to one image (tensor on GPU -> HIP kernels; numpy / CPU
    tensor -> the threaded host executor, bit-identical to the golden path).
    A 4-D BxHxWxC input is a batch of frames; the result stacks the frames."""
    if image.ndim == 4:
        if image.shape[3] not in (1, 3):
            raise ValueError(f"a batch must be BxHxWxC with C in (1, 3), got {tuple(image.shape)}")
        outs = [apply(image[b], chain, border, fuse) for b in range(image.shape[0])]
        if _is_tensor(image):
            return torch.stack(outs) if outs else image.new_empty((0,) + tuple(image.shape[1:]))
        return np.stack(outs) if outs else np.empty((0,) + tuple(image.shape[1:]), np.uint8)
    if _is_tensor(image) and image.is_cuda:
        if image.dtype != torch.uint8:
            raise TypeError("image tensor must be uint8")
        x = image.contiguous()
        W, H, Cc = _shape(x)
        if Cc == 1 and x.ndim == 3:
            x = x.reshape(H, W)
        eng = _engine(W, H, Cc, chain, border, fuse, x.device.index)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        cout = eng.out_channels
        out = torch.empty((H, W) if cout == 1 else (H, W, cout), dtype=torch.uint8, device=x.device)
        with eng._lock:
            if eng._stream != stream:
                # the new stream waits for the work still queued on the old one
                eng.use_external_stream(stream)
                eng._stream = stream
            eng.load_packed_ptr(x.data_ptr(), True)
            eng.run(1)
            eng.store_packed_ptr(out.data_ptr(), True)
        # keep x alive until the stream has consumed it
        x.record_stream(torch.cuda.current_stream(x.device))
        return out
    was_tensor = _is_tensor(image)
    arr = image.numpy() if was_tensor else np.asarray(image)
    if arr.dtype != np.uint8:
        raise TypeError("image must be uint8")
    if arr.ndim == 3 and arr.shape[2] == 1:
        arr = arr[:, :, 0]
    out = C.cpu_apply(np.ascontiguousarray(arr), chain, border, fuse)
    return torch.from_numpy(out) if was_tensor else out


def reference(image, chain: str, border: str = "reflect101"):
    """Golden CPU result of `chain`, applied op by op (no fusion)."""
    arr = image.detach().cpu().numpy() if _is_tensor(image) else np.asarray(image)
    return C.golden_apply_unfused(np.ascontiguousarray(arr), chain, border)


# ---- named convenience wrappers -------------------------------------------------
def grayscale(x, mode: str = "bt601"):
    return apply(x, f"gray:{mode}")


def contrast(x, factor: float = 3.5, rounding: str = "ref"):
    return apply(x, f"contrast:{factor}:{rounding}")


def invert(x):
    return apply(x, "invert")


def brightness(x, delta: int):
    return apply(x, f"brightness:{int(delta)}")


def threshold(x, t: int = 128):
    return apply(x, f"threshold:{int(t)}")


def gaussian_blur(x, ksize: int = 5, border: str = "reflect101"):
    if ksize in (3, 5, 7):
        return apply(x, f"gaussian{ksize}", border)
    return apply(x, f"blur:{ksize}", border)


def box_blur(x, ksize: int = 3, border: str = "reflect101"):
    return apply(x, f"box{ksize}", border)


def sobel(x, border: str = "reflect101"):
    return apply(x, "sobel", border)


def sharpen(x, border: str = "reflect101"):
    return apply(x, "sharpen", border)


def laplace(x, border: str = "reflect101"):
    return apply(x, "laplace", border)


def emboss(x, size: int = 3, border: str = "reflect101"):
    return apply(x, f"emboss{size}", border)


def median(x, k: int = 3, border: str = "reflect101"):
    return apply(x, f"median{int(k)}", border)


def bilateral(x, sigma: float = 25.0, ksize: int = 5, border: str = "reflect101"):
    """Bilateral filter, per channel: ksize 3 or 5, sigma the range sigma in grey levels."""
    if int(ksize) not in (3, 5):
        raise ValueError(f"bilateral window size must be 3 or 5, got {ksize}")
    return apply(x, f"bilateral{int(ksize)}:{float(sigma)!r}", border)


def erode(x, k: int = 3, border: str = "reflect101"):
    return apply(x, f"erode{int(k)}", border)


def dilate(x, k: int = 3, border: str = "reflect101"):
    return apply(x, f"dilate{int(k)}", border)


def morph_open(x, k: int = 3, border: str = "reflect101"):
    return apply(x, f"open{int(k)}", border)


def morph_close(x, k: int = 3, border: str = "reflect101"):
    return apply(x, f"close{int(k)}", border)


def conv2d(x, weights, border: str = "reflect101"):
    """Generic KxK float correlation on the MFMA path (weights: KxK array)."""
    w = np.asarray(weights, dtype=np.float64)
    K = w.shape[0]
    if w.shape != (K, K) or K % 2 == 0:
        raise ValueError("weights must be an odd KxK matrix")
    spec = ";".join(repr(float(v)) for v in w.reshape(-1))
    return apply(x, f"conv:{K}:{spec}", border)


def sep_conv2d(x, h, v, border: str = "reflect101"):
    """Rank-one KxK correlation, weights[dy][dx] = v[dy] * h[dx] (separable MFMA path)."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    K = h.shape[0]
    if v.shape[0] != K or K % 2 == 0:
        raise ValueError("h and v must have the same odd length")
    hs = ";".join(repr(float(t)) for t in h)
    vs = ";".join(repr(float(t)) for t in v)
    return apply(x, f"sepconv:{K}:{hs}:{vs}", border)


def color_matrix(x, M, offset=None):
    """3x3 colour matrix (and optional 3 offsets) on an RGB image: out_c = sum_k M[c][k] in_k + offset_c,
    evaluated in Q12 fixed point (`C.color_matrix(token)` shows the quantised coefficients)."""
    m = np.asarray(M, dtype=np.float64)
    if m.shape != (3, 3):
        raise ValueError("M must be a 3x3 matrix")
    spec = ";".join(repr(float(v)) for v in m.reshape(-1))
    if offset is not None:
        b = np.asarray(offset, dtype=np.float64).reshape(-1)
        if b.shape != (3,):
            raise ValueError("offset must have 3 entries")
        spec += ":" + ";".join(repr(float(v)) for v in b)
    return apply(x, f"colormatrix:{spec}")


def sepia(x):
    return apply(x, "sepia")


def saturation(x, s: float):
    return apply(x, f"saturation:{float(s)!r}")


def swap_rb(x):
    return apply(x, "swaprb")


def rgb_to_ycbcr(x):
    return apply(x, "ycbcr")


def ycbcr_to_rgb(x):
    return apply(x, "ycbcr:inv")


def large_blur(x, ksize: int = 31, sigma: float = 0.0, border: str = "reflect101"):
    return apply(x, f"blur:{ksize}:{sigma}" if sigma > 0 else f"blur:{ksize}", border)


# ---- histogram and the statistic ops ---------------------------------------------
def histogram(image):
    """Per-channel histogram: an int64 numpy array of shape (C, 256) (C = 1 or 3) counting exactly the
    image's H x W pixels.  A CUDA tensor is counted by the k_hist HIP kernel on torch's current stream
    (through the cached engine, like `apply`); a numpy array / CPU tensor by the threaded host executor.
    A BxHxWxC batch gives (B, C, 256)."""
    if image.ndim == 4:
        if image.shape[3] not in (1, 3):
            raise ValueError(f"a batch must be BxHxWxC with C in (1, 3), got {tuple(image.shape)}")
        hs = [histogram(image[b]) for b in range(image.shape[0])]
        return np.stack(hs) if hs else np.empty((0, image.shape[3], 256), np.int64)
    if _is_tensor(image) and image.is_cuda:
        if image.dtype != torch.uint8:
            raise TypeError("image tensor must be uint8")
        x = image.contiguous()
        W, H, Cc = _shape(x)
        # any chain does: the engine only holds the padded stripe the kernel reads
        eng = _engine(W, H, Cc, "invert", "reflect101", True, x.device.index)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        with eng._lock:
            if eng._stream != stream:
                eng.use_external_stream(stream)
                eng._stream = stream
            eng.load_packed_ptr(x.data_ptr(), True)
            h = eng.histogram(False)  # synchronises the stream: x has been consumed
        return h
    arr = image.numpy() if _is_tensor(image) else np.asarray(image)
    if arr.dtype != np.uint8:
        raise TypeError("image must be uint8")
    if arr.ndim == 3 and arr.shape[2] == 1:
        arr = arr[:, :, 0]
    _shape(arr)
    return C.cpu_histogram(np.ascontiguousarray(arr))


def equalize(x):
    """Histogram equalisation (one table from the pooled channels, `FILTERS['equalize']`)."""
    return apply(x, "equalize")


def autocontrast(x, cutoff: float = 0.0):
    """Contrast stretch clipping `cutoff` percent of the pixels at each end (0 <= cutoff < 50)."""
    return apply(x, f"autocontrast:{float(cutoff)!r}")


def threshold_otsu(x):
    """Binarise at Otsu's level of the image's own histogram."""
    return apply(x, "threshold:otsu")


def otsu_level(x) -> int:
    """Otsu's level T in [1, 255] of the image (channels pooled): threshold_otsu(x) == (x >= T) * 255."""
    return int(C.otsu_level(histogram(x)))


# ---- two-image ops -------------------------------------------------------------
def unsharp_mask(x, amount: float = 1.0, ksize: int = 5, border: str = "reflect101"):
    """x + amount * (x - gaussian_ksize(x)) in Q12 fixed point (`FILTERS['unsharp[:S[:K]]']`)."""
    return apply(x, f"unsharp:{float(amount)!r}:{int(ksize)}", border)


def morph_gradient(x, k: int = 3, border: str = "reflect101"):
    """dilate_k(x) - erode_k(x)."""
    return apply(x, f"gradient{int(k)}", border)


def top_hat(x, k: int = 3, border: str = "reflect101"):
    """x - open_k(x)."""
    return apply(x, f"tophat{int(k)}", border)


def black_hat(x, k: int = 3, border: str = "reflect101"):
    """close_k(x) - x."""
    return apply(x, f"blackhat{int(k)}", border)


def adaptive_threshold(x, ksize: int = 3, c: int = 0, border: str = "reflect101"):
    """x > box_ksize(x) - c ? 255 : 0 (OpenCV's ADAPTIVE_THRESH_MEAN_C on box's own rounding); ksize 3 or 5, for
    larger windows see `local_threshold`."""
    return apply(x, f"threshold:adaptive:{int(ksize)}:{int(c)}", border)


def combine(x, y, op: str, border: str = "reflect101"):
    """Run the chain `op` on x with y as the held image: a combine token (add, sub, rsub, absdiff, min, max,
    lincomb:a:b[:c], blend:t, above[:d]) or any chain that reads the held image.  x and y have the same
    shape; CUDA tensors run on the k_combine HIP kernel, numpy arrays / CPU tensors on the host executor."""
    if tuple(x.shape) != tuple(y.shape):
        raise ValueError(f"combine needs two images of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.ndim == 4:
        outs = [combine(x[b], y[b], op, border) for b in range(x.shape[0])]
        if _is_tensor(x):
            return torch.stack(outs) if outs else x.new_empty(tuple(x.shape))
        return np.stack(outs) if outs else np.empty(tuple(x.shape), np.uint8)
    if _is_tensor(x) and x.is_cuda:
        if not (_is_tensor(y) and y.is_cuda and y.device == x.device):
            raise ValueError("combine needs both tensors on the same GPU")
        if x.dtype != torch.uint8 or y.dtype != torch.uint8:
            raise TypeError("image tensors must be uint8")
        xc, yc = x.contiguous(), y.contiguous()
        W, H, Cc = _shape(xc)
        eng = _engine(W, H, Cc, op, border, True, xc.device.index, held=True)
        stream = torch.cuda.current_stream(xc.device).cuda_stream
        cout = eng.out_channels
        out = torch.empty((H, W) if cout == 1 else (H, W, cout), dtype=torch.uint8, device=xc.device)
        with eng._lock:
            if eng._stream != stream:
                eng.use_external_stream(stream)
                eng._stream = stream
            eng.load_packed_ptr(xc.data_ptr(), True)
            eng.load_held_packed_ptr(yc.data_ptr(), True)
            eng.run(1)
            eng.store_packed_ptr(out.data_ptr(), True)
        xc.record_stream(torch.cuda.current_stream(xc.device))
        yc.record_stream(torch.cuda.current_stream(xc.device))
        return out
    was_tensor = _is_tensor(x)
    ax = x.numpy() if was_tensor else np.asarray(x)
    ay = y.numpy() if _is_tensor(y) else np.asarray(y)
    if ax.dtype != np.uint8 or ay.dtype != np.uint8:
        raise TypeError("images must be uint8")
    if ax.ndim == 3 and ax.shape[2] == 1:
        ax, ay = ax[:, :, 0], ay[:, :, 0]
    out = C.cpu_apply(np.ascontiguousarray(ax), op, border, True, 0, np.ascontiguousarray(ay))
    return torch.from_numpy(out) if was_tensor else out


def absdiff(x, y):
    return combine(x, y, "absdiff")


def add(x, y):
    """min(255, x + y)."""
    return combine(x, y, "add")


def subtract(x, y):
    """max(0, x - y)."""
    return combine(x, y, "rsub")


def blend(x, y, t: float):
    """t x + (1 - t) y in Q12 fixed point, 0 <= t <= 1."""
    return combine(x, y, f"blend:{float(t)!r}")


def minimum(x, y):
    return combine(x, y, "min")


def maximum(x, y):
    return combine(x, y, "max")


# ---- whole-frame stages in front of the chain: one driver for resize, orient, warp and remap ----
def _packed_frame(arr, fn):
    """fn on arr as the packed array the C++ layer takes (HxWx1 goes in as HxW); the result keeps arr's rank."""
    keep = arr.ndim == 3 and arr.shape[2] == 1
    out = fn(np.ascontiguousarray(arr[:, :, 0] if keep else arr))
    return out[:, :, None] if keep else out


def _reference_frame(x, golden):
    """The golden loop of a stage on x as a numpy array: golden(W, H) gives the function of the packed array."""
    arr = x.detach().cpu().numpy() if _is_tensor(x) else np.asarray(x)
    W, H, _ = _shape(arr)
    return _packed_frame(arr, golden(W, H))


def _frame_stage(x, plan, on_device, on_host, pitched=True):
    """One frame, or a BxHxWxC batch frame by frame, through a whole-frame stage.

    plan(W, H) -> (W2, H2, args): the destination size and whatever the two calls need.
    on_device(view, W2, H2, args, stream) makes the C.*_device call on torch's current stream; view is its
    leading arguments (src, src_pitch, W, H, C, dst, dst_pitch); it returns the tensors besides the input
    that must outlive the queued work, or None.  pitched: the kernel reads a strided view in place as long
    as a row's pixels are packed; otherwise the input is made contiguous.
    on_host(arr, W2, H2, args) makes the C.cpu_* call on a packed numpy array.
    The result has x's container and rank."""
    if x.ndim == 4:
        if x.shape[3] not in (1, 3):
            raise ValueError(f"a batch must be BxHxWxC with C in (1, 3), got {tuple(x.shape)}")
        outs = [_frame_stage(x[b], plan, on_device, on_host, pitched) for b in range(x.shape[0])]
        if outs:
            return torch.stack(outs) if _is_tensor(x) else np.stack(outs)
        W2, H2, _ = plan(x.shape[2], x.shape[1])
        shape = (0, H2, W2, x.shape[3])
        return x.new_empty(shape) if _is_tensor(x) else np.empty(shape, np.uint8)
    W, H, Cc = _shape(x)
    W2, H2, args = plan(W, H)
    if _is_tensor(x) and x.is_cuda:
        if x.dtype != torch.uint8:
            raise TypeError("image tensor must be uint8")
        packed = pitched and x.stride(1) == Cc and (x.ndim == 2 or x.stride(2) == 1) and x.stride(0) >= W * Cc
        xc = x if packed else x.contiguous()
        out = torch.empty((H2, W2) + tuple(x.shape[2:]), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream(x.device)
            view = (xc.data_ptr(), xc.stride(0) if pitched else W * Cc, W, H, Cc, out.data_ptr(), W2 * Cc)
            extra = on_device(view, W2, H2, args, stream) or ()
        # keep the input (and the stage's own tensors) alive until the stream has consumed them
        for t in (xc, *extra):
            t.record_stream(stream)
        return out
    was_tensor = _is_tensor(x)
    arr = x.numpy() if was_tensor else np.asarray(x)
    if arr.dtype != np.uint8:
        raise TypeError("image must be uint8")
    out = _packed_frame(arr, lambda a: on_host(a, W2, H2, args))
    return torch.from_numpy(out) if was_tensor else out


# ---- resize: a stage in front of the chain, not a chain token ---------------------
RESIZE_MODES = ("auto", "nearest", "bilinear", "area")
_MAX_SIZE = 65535


def _resize_target(H, W, size, scale):
    if (size is None) == (scale is None):
        raise ValueError("resize needs exactly one of size=(H2, W2) and scale")
    if size is not None:
        try:
            H2, W2 = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError(f"size must be (H2, W2), got {size!r}") from None
    else:
        sy, sx = (scale, scale) if np.isscalar(scale) else scale
        if not (sy > 0 and sx > 0):
            raise ValueError(f"scale must be positive, got {scale!r}")
        H2, W2 = max(1, int(np.rint(H * sy))), max(1, int(np.rint(W * sx)))
    if not (1 <= H2 <= _MAX_SIZE and 1 <= W2 <= _MAX_SIZE):
        raise ValueError(f"size must lie in 1..{_MAX_SIZE} per axis, got ({H2}, {W2})")
    return H2, W2


def resize(x, size=None, scale=None, mode: str = "auto"):
    """Resize an image to size=(H2, W2), or by scale (a float or (sy, sx); n_out = max(1, rint(n * s))).

    mode: "nearest", "bilinear" (half-pixel centres, no antialiasing), "area" (exact cell overlap,
    shrinking axes only, factor <= 32) or "auto" (per axis: area where it shrinks, bilinear where it
    grows).  One integer rule in every layer (`C.resize_taps`): CUDA uint8 tensors run on the k_resize
    HIP kernel on torch's current stream, numpy arrays / CPU tensors on the threaded host executor,
    bit-identical to `resize_reference`.  A BxHxWxC batch runs frame by frame."""
    if mode not in RESIZE_MODES:
        raise ValueError(f"mode must be one of {RESIZE_MODES}, got {mode!r}")

    def plan(W, H):
        H2, W2 = _resize_target(H, W, size, scale)
        return W2, H2, None
    return _frame_stage(x, plan,
                        lambda view, W2, H2, _, stream: C.resize_device(*view, W2, H2, mode, stream.cuda_stream),
                        lambda arr, W2, H2, _: C.cpu_resize(arr, W2, H2, mode), pitched=False)


def resize_reference(x, size=None, scale=None, mode: str = "auto"):
    """Golden CPU result of `resize`: the rule as a plain per-pixel loop."""
    def golden(W, H):
        H2, W2 = _resize_target(H, W, size, scale)
        return lambda arr: C.golden_resize(arr, W2, H2, mode)
    return _reference_frame(x, golden)


# ---- orientation and crop: a stage in front of the chain, not a chain token ---------
ORIENTATIONS = tuple(C.orient_names())


def _crop_tuple(crop):
    if crop is None:
        return None
    try:
        x0, y0, w, h = (int(v) for v in crop)
    except (TypeError, ValueError):
        raise ValueError(f"crop must be (x0, y0, w, h), got {crop!r}") from None
    return x0, y0, w, h


def _oriented_shape(H, W, name, crop):
    oh, ow = (W, H) if C.parse_orient(name)[1] & 4 else (H, W)
    if crop is None:
        return oh, ow
    x0, y0, w, h = crop
    if not (w >= 1 and h >= 1 and x0 >= 0 and y0 >= 0 and x0 + w <= ow and y0 + h <= oh):
        raise ValueError(f"crop {w}x{h}+{x0}+{y0} is empty or leaves the oriented frame of {ow}x{oh}")
    return h, w


def orient(x, op: str = "none", crop=None):
    """One of the eight orientations of the rectangle, then an optional crop, in one pass.

    op: "none", "fliph", "rot180", "flipv", "transpose", "rot90" (clockwise, alias "cw"),
    "transverse", "rot270" (alias "ccw") or "exif:N" (the operation that shows an image stored with
    Exif Orientation N upright).  crop=(x0, y0, w, h) is a window of the oriented frame.  CUDA uint8
    tensors run on the k_orient HIP kernel on torch's current stream (rows of a strided view are
    read in place), numpy arrays / CPU tensors on the threaded host executor, bit-identical to
    `orient_reference`.  A BxHxWxC batch runs frame by frame."""
    name = C.parse_orient(op)[0]
    crop = _crop_tuple(crop)

    def plan(W, H):
        H2, W2 = _oriented_shape(H, W, name, crop)
        return W2, H2, None
    return _frame_stage(x, plan,
                        lambda view, W2, H2, _, stream: C.orient_device(*view, name, crop, stream.cuda_stream),
                        lambda arr, W2, H2, _: C.cpu_orient(arr, name, crop))


def orient_reference(x, op: str = "none", crop=None):
    """Golden CPU result of `orient`: the rule as a plain per-pixel loop."""
    return _reference_frame(
        x, lambda W, H: lambda arr: C.golden_orient(arr, C.parse_orient(op)[0], _crop_tuple(crop)))


def flip(x, axis):
    """Flip along axis 0 (rows: `flipv`), axis 1 (columns: `fliph`) or both, (0, 1) (`rot180`)."""
    axes = (axis,) if np.isscalar(axis) else tuple(axis)
    if not axes or any(a not in (0, 1) for a in axes) or len(set(axes)) != len(axes):
        raise ValueError(f"axis must be 0, 1 or (0, 1), got {axis!r}")
    return orient(x, {(0,): "flipv", (1,): "fliph"}.get(axes, "rot180"))


def rot90(x, k: int = 1):
    """k counter-clockwise quarter turns, like np.rot90 / torch.rot90 on the first two axes (any integer k)."""
    return orient(x, ("none", "rot270", "rot180", "rot90")[int(k) % 4])


def transpose_image(x):
    """Rows become columns (`transpose`)."""
    return orient(x, "transpose")


def crop(x, x0, y0, w, h):
    """The window of w x h pixels whose top-left pixel is (x0, y0)."""
    return orient(x, "none", (x0, y0, w, h))


def exif_orientation(path_or_bytes) -> int:
    """Exif Orientation (1..8) of a JPEG file or byte string; 1 when it carries none (or is no JPEG)."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    return C.jpeg_orientation(data)


# ---- affine warp: a stage in front of the chain (after orient / crop, before resize) ----
WARP_MODES = ("bilinear", "nearest")
WARP_BORDERS = ("constant", "replicate")


def _warp_map(W, H, M, size, inverse):
    """The quantised map of a 2x3 matrix: (W2, H2, [A00, A01, B0, A10, A11, B1])."""
    try:
        vals = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(-1)]
    except (TypeError, ValueError):
        raise ValueError(f"M must be a 2x3 matrix of numbers, got {M!r}") from None
    if len(vals) != 6:
        raise ValueError(f"M must be a 2x3 matrix (six numbers), got {len(vals)}")
    if size is None:
        H2, W2 = H, W
    else:
        try:
            H2, W2 = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError(f"size must be (H2, W2), got {size!r}") from None
    if not (1 <= W2 <= 65535 and 1 <= H2 <= 65535):
        raise ValueError(f"warp: destination size {W2}x{H2} outside 1..65535")
    try:
        q = C.warp_quantise(vals, bool(inverse), W, H, W2, H2)
    except RuntimeError as e:
        raise ValueError(str(e)) from None
    return q[6], q[7], list(q[:6])


def _warp_args(mode, border, fill):
    if mode not in WARP_MODES:
        raise ValueError(f"warp: unknown mode {mode!r} (bilinear | nearest)")
    if border not in WARP_BORDERS:
        raise ValueError(f"warp: unknown border {border!r} (constant | replicate)")
    if isinstance(fill, bool) or int(fill) != fill or not 0 <= int(fill) <= 255:
        raise ValueError(f"warp: fill must be an integer in 0..255, got {fill!r}")
    return mode, border, int(fill)


def _warp_frame(x, mapper, mode, border, fill):
    """One frame (or a batch, frame by frame) through k_warp / cpu_warp; mapper(W, H) -> (W2, H2, q)."""
    return _frame_stage(
        x, mapper,
        lambda view, W2, H2, q, stream: C.warp_device(*view, q, W2, H2, mode, border, fill, stream.cuda_stream),
        lambda arr, W2, H2, q: C.cpu_warp(arr, q, W2, H2, mode, border, fill))


def warp_affine(x, M, size=None, mode: str = "bilinear", border: str = "constant", fill: int = 0,
                inverse: bool = False):
    """Affine warp by the forward 2x3 matrix M (source -> destination, like cv2.warpAffine without
    WARP_INVERSE_MAP; inverse=True: M maps destination to source itself).

    size=(H2, W2) is the destination (default: the source's).  Integer indices are pixel centres.  The
    inverse map is quantised to Q24 once; every pixel follows from it in integers, so CUDA uint8 tensors
    (the k_warp HIP kernel on torch's current stream; rows of a strided view are read in place), numpy
    arrays / CPU tensors (the threaded host executor) and `warp_reference` agree bit for bit.  Taps
    outside the frame are `fill` (border="constant") or the clamped pixel ("replicate").  A map that
    shrinks is not antialiased.  A BxHxWxC batch runs frame by frame."""
    mode, border, fill = _warp_args(mode, border, fill)
    return _warp_frame(x, lambda W, H: _warp_map(W, H, M, size, inverse), mode, border, fill)


def _rotation_mapper(angle, expand):
    def mapper(W, H):
        try:
            minv, W2, H2 = C.rotate_matrix(float(angle), bool(expand), W, H)
        except RuntimeError as e:
            raise ValueError(str(e)) from None
        return _warp_map(W, H, minv, (H2, W2), True)
    return mapper


def rotate(x, angle: float, expand: bool = False, mode: str = "bilinear", border: str = "constant", fill: int = 0):
    """Rotation by `angle` degrees, counter-clockwise as seen (cv2.getRotationMatrix2D, PIL), about the
    frame's centre.  expand=True grows the frame to hold the whole rotated image (multiples of 90 are then
    exact quarter turns); otherwise the size is kept.  See `warp_affine`."""
    mode, border, fill = _warp_args(mode, border, fill)
    return _warp_frame(x, _rotation_mapper(angle, expand), mode, border, fill)


def warp_reference(x, M, size=None, mode: str = "bilinear", border: str = "constant", fill: int = 0,
                   inverse: bool = False):
    """Golden CPU result of `warp_affine`: the rule as a plain per-pixel loop."""
    mode, border, fill = _warp_args(mode, border, fill)
    def golden(W, H):
        W2, H2, q = _warp_map(W, H, M, size, inverse)
        return lambda arr: C.golden_warp(arr, q, W2, H2, mode, border, fill)
    return _reference_frame(x, golden)


# ---- mesh warp: perspective, undistort, remap (the affine warp's slot in front of the chain) ----
MESH_SPACINGS = (1, 2, 4, 8, 16, 32, 64)
_NODE_LIMIT = 1 << 30  # 2^18 pixels in Q12


def _mesh_grid(n, spacing):
    return ((n - 1) >> (spacing.bit_length() - 1)) + 2


def _check_spacing(spacing):
    if isinstance(spacing, bool) or spacing not in MESH_SPACINGS:
        raise ValueError(f"remap: spacing {spacing!r} is not a power of two in 1..64")
    return int(spacing)


def _dest_size(size, W, H):
    if size is None:
        return W, H
    try:
        H2, W2 = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (H2, W2), got {size!r}") from None
    if not (1 <= W2 <= 65535 and 1 <= H2 <= 65535):
        raise ValueError(f"remap: destination size {W2}x{H2} outside 1..65535")
    return W2, H2


def _check_mesh(mesh, spacing, W2, H2):
    """An int32 mesh of shape (gh, gw, 2) with every node inside (-2^18, 2^18) pixels; numpy or tensor."""
    want = (_mesh_grid(H2, spacing), _mesh_grid(W2, spacing), 2)
    if _is_tensor(mesh):
        if mesh.dtype != torch.int32:
            raise TypeError("the mesh must be int32")
        if tuple(mesh.shape) != want:
            raise ValueError(f"remap: a mesh of spacing {spacing} for {W2}x{H2} has shape "
                             f"{want[0]}x{want[1]}x2, got {tuple(mesh.shape)}")
        if mesh.numel() and int(mesh.abs().max()) >= _NODE_LIMIT:  # (int32 min wraps to itself: negative, caught below)
            raise ValueError("remap: a node lies at or beyond 2^18 pixels")
        if mesh.numel() and int(mesh.min()) <= -_NODE_LIMIT:
            raise ValueError("remap: a node lies at or beyond 2^18 pixels")
        return mesh.contiguous()
    mesh = np.asarray(mesh)
    if mesh.dtype != np.int32:
        raise TypeError("the mesh must be int32")
    if mesh.shape != want:
        raise ValueError(f"remap: a mesh of spacing {spacing} for {W2}x{H2} has shape "
                         f"{want[0]}x{want[1]}x2, got {mesh.shape}")
    if mesh.size and (int(mesh.max()) >= _NODE_LIMIT or int(mesh.min()) <= -_NODE_LIMIT):
        raise ValueError("remap: a node lies at or beyond 2^18 pixels")
    return np.ascontiguousarray(mesh)


def _remap_frame(x, mesher, mode, border, fill):
    """One frame (or a batch, frame by frame) through k_remap / cpu_remap; mesher(W, H) -> (W2, H2, (mesh,
    spacing)), the mesh a checked int32 array or tensor."""
    def on_device(view, W2, H2, args, stream):
        mesh, spacing = args
        if _is_tensor(mesh):
            dm = mesh.to(stream.device).contiguous()
        else:
            dm = torch.from_numpy(mesh).to(stream.device, non_blocking=False)
        C.remap_device(*view, dm.data_ptr(), dm.numel(), spacing, W2, H2, mode, border, fill, stream.cuda_stream)
        return (dm,)

    def on_host(arr, W2, H2, args):
        mesh, spacing = args
        hm = mesh.cpu().numpy() if _is_tensor(mesh) else mesh
        return C.cpu_remap(arr, hm, spacing, W2, H2, mode, border, fill)
    return _frame_stage(x, mesher, on_device, on_host)


def _builder(fn, *args):
    try:
        return fn(*args)
    except RuntimeError as e:
        raise ValueError(str(e)) from None


def _matrix9(Hm):
    try:
        vals = [float(v) for v in np.asarray(Hm, dtype=np.float64).reshape(-1)]
    except (TypeError, ValueError):
        raise ValueError(f"H must be a 3x3 matrix of numbers, got {Hm!r}") from None
    if len(vals) != 9:
        raise ValueError(f"H must be a 3x3 matrix (nine numbers), got {len(vals)}")
    return vals


def _perspective_mesher(Hm, size, inverse):
    vals = _matrix9(Hm)

    def mesher(W, H):
        W2, H2 = _dest_size(size, W, H)
        return W2, H2, _builder(C.perspective_mesh, vals, bool(inverse), W, H, W2, H2, 0)
    return mesher


def mesh_warp(x, mesh, spacing: int, size=None, mode: str = "bilinear", border: str = "constant", fill: int = 0):
    """Warp by a mesh: an int32 array or tensor of shape (gh, gw, 2) that holds the source position (x, y) in
    Q12 of the destination pixels (j * spacing, i * spacing), gw = ((W2 - 1) // spacing) + 2, gh likewise;
    between the nodes the position is interpolated bilinearly, in integers (`remap.h`).  size=(H2, W2) is the
    destination (default: the source's).  CUDA uint8 tensors run the k_remap HIP kernel on torch's current
    stream (a CUDA mesh is used where it lives), numpy arrays / CPU tensors the threaded host executor;
    they and `remap_reference` agree bit for bit.  A BxHxWxC batch runs frame by frame."""
    mode, border, fill = _warp_args(mode, border, fill)
    spacing = _check_spacing(spacing)
    checked = {}

    def mesher(W, H):
        W2, H2 = _dest_size(size, W, H)
        if (W2, H2) not in checked:
            checked[(W2, H2)] = _check_mesh(mesh, spacing, W2, H2)
        return W2, H2, (checked[(W2, H2)], spacing)
    return _remap_frame(x, mesher, mode, border, fill)


def warp_perspective(x, H, size=None, mode: str = "bilinear", border: str = "constant", fill: int = 0,
                     inverse: bool = False):
    """Perspective warp by the forward 3x3 matrix H (source -> destination, like cv2.warpPerspective without
    WARP_INVERSE_MAP; inverse=True: H maps destination to source itself).  The map is evaluated in double at
    the nodes of a mesh whose spacing is chosen to keep the interpolation within 2^-10 pixel; see
    `mesh_warp`.  A destination the horizon crosses is refused."""
    mode, border, fill = _warp_args(mode, border, fill)
    return _remap_frame(x, _perspective_mesher(H, size, inverse), mode, border, fill)


def perspective_from_points(src, dst):
    """cv2.getPerspectiveTransform: the forward 3x3 matrix (h22 = 1) that maps the four points src[k] = (x, y)
    to dst[k]."""
    try:
        s = [float(v) for v in np.asarray(src, dtype=np.float64).reshape(-1)]
        d = [float(v) for v in np.asarray(dst, dtype=np.float64).reshape(-1)]
    except (TypeError, ValueError):
        raise ValueError("perspective_from_points: four points (x, y) each") from None
    if len(s) != 8 or len(d) != 8:
        raise ValueError("perspective_from_points: four points (x, y) each")
    return np.asarray(_builder(C.perspective_from_points, s, d), np.float64).reshape(3, 3)


def rectify_quad(x, quad, size=None, mode: str = "bilinear", border: str = "constant", fill: int = 0):
    """The quadrilateral quad = (TL, TR, BR, BL), points (x, y) of the source, straightened to a rectangle
    whose corners they become.  size=(H2, W2); default: the longer of each pair of opposite sides, rounded,
    plus one."""
    mode, border, fill = _warp_args(mode, border, fill)
    try:
        pts = [float(v) for v in np.asarray(quad, dtype=np.float64).reshape(-1)]
    except (TypeError, ValueError):
        raise ValueError("rectify_quad: four points (x, y)") from None
    if len(pts) != 8:
        raise ValueError("rectify_quad: four points (x, y)")
    if size is None:
        Hm, W2, H2 = _builder(C.quad_matrix, pts, 0, 0)
    else:
        W2, H2 = _dest_size(size, 1, 1)
        Hm, W2, H2 = _builder(C.quad_matrix, pts, W2, H2)
    return _remap_frame(x, _perspective_mesher(Hm, (H2, W2), False), mode, border, fill)


def undistort(x, k1: float, k2: float = 0.0, f=None, center=None, mode: str = "bilinear", border: str = "constant",
              fill: int = 0):
    """Radial lens undistortion (cv2.undistort with K = newK = [[f, 0, cx], [0, f, cy]] and
    dist = (k1, k2, 0, 0)); f defaults to half the diagonal, center to ((W - 1) / 2, (H - 1) / 2)."""
    mode, border, fill = _warp_args(mode, border, fill)
    ff = None if f is None else float(f)
    cc = None if center is None else [float(v) for v in center]

    def mesher(W, H):
        return W, H, _builder(C.radial_mesh, float(k1), float(k2), ff, cc, W, H, 0)
    return _remap_frame(x, mesher, mode, border, fill)


def _quantise_maps(map_x, map_y):
    """round(4096 m) of two float maps, padded by one replicated row and column: the mesh of spacing 1."""
    if _is_tensor(map_x) != _is_tensor(map_y):
        raise TypeError("remap: map_x and map_y must both be tensors or both arrays")
    if _is_tensor(map_x):
        if map_x.shape != map_y.shape or map_x.ndim != 2 or map_x.device != map_y.device:
            raise ValueError("remap: map_x and map_y must be two H2 x W2 maps on one device")
        if not (map_x.is_floating_point() and map_y.is_floating_point()):
            raise TypeError("remap: the maps must be floating point")
        m = torch.stack([map_x, map_y], dim=2).to(torch.float64)
        if m.numel() and not bool(torch.isfinite(m).all()):
            raise ValueError("remap: non-finite number in the maps")
        q = torch.round(m * 4096.0)
        if q.numel() and float(q.abs().max()) >= _NODE_LIMIT:
            raise ValueError("remap: a node lies at or beyond 2^18 pixels")
        q = q.to(torch.int32)
        q = torch.cat([q, q[-1:]], dim=0)
        return torch.cat([q, q[:, -1:]], dim=1).contiguous()
    mx, my = np.asarray(map_x), np.asarray(map_y)
    if mx.shape != my.shape or mx.ndim != 2:
        raise ValueError("remap: map_x and map_y must be two H2 x W2 maps")
    if mx.dtype.kind != "f" or my.dtype.kind != "f":
        raise TypeError("remap: the maps must be floating point")
    m = np.stack([mx, my], axis=2).astype(np.float64)
    if not np.isfinite(m).all():
        raise ValueError("remap: non-finite number in the maps")
    q = np.rint(m * 4096.0)
    if q.size and np.abs(q).max() >= _NODE_LIMIT:
        raise ValueError("remap: a node lies at or beyond 2^18 pixels")
    return np.pad(q.astype(np.int32), ((0, 1), (0, 1), (0, 0)), mode="edge")


def remap(x, map_x, map_y, mode: str = "bilinear", border: str = "constant", fill: int = 0):
    """cv2.remap: out[y, x] = in(map_y[y, x], map_x[y, x]) for two float maps of the destination's size
    (integer values are pixel centres).  The maps are quantised to Q12 where they live (CUDA maps on the
    device) and run as a mesh of spacing 1, where nothing is interpolated; see `mesh_warp`."""
    mode, border, fill = _warp_args(mode, border, fill)
    mesh = _quantise_maps(map_x, map_y)
    H2, W2 = mesh.shape[0] - 1, mesh.shape[1] - 1
    if not (1 <= W2 <= 65535 and 1 <= H2 <= 65535):
        raise ValueError(f"remap: destination size {W2}x{H2} outside 1..65535")
    return _remap_frame(x, lambda W, H: (W2, H2, (mesh, 1)), mode, border, fill)


def remap_reference(x, mesh, spacing: int, size=None, mode: str = "bilinear", border: str = "constant",
                    fill: int = 0):
    """Golden CPU result of `mesh_warp`: the rule as a plain per-pixel loop."""
    mode, border, fill = _warp_args(mode, border, fill)
    spacing = _check_spacing(spacing)

    def golden(W, H):
        W2, H2 = _dest_size(size, W, H)
        hm = _check_mesh(mesh.cpu() if _is_tensor(mesh) else mesh, spacing, W2, H2)
        hm = hm.numpy() if _is_tensor(hm) else hm
        return lambda arr: _builder(C.golden_remap, arr, hm, spacing, W2, H2, mode, border, fill)
    return _reference_frame(x, golden)


# ---- connected components (csrc/include/stripe/components.h): labels, stats, area filter ----
STAT_COLUMNS = tuple(C.STAT_COLUMNS)


def _mask_shape(x):
    """(W, H) of a mask HxW or HxWx1; an RGB frame and every other shape is refused."""
    if x.ndim == 4:
        raise ValueError(f"components: one frame at a time, got a batch of shape {tuple(x.shape)}")
    if x.ndim == 3 and x.shape[2] == 3:
        raise ValueError("components: needs a 1-channel image, got C = 3; convert first (gray, threshold, ...)")
    if x.ndim == 2 or (x.ndim == 3 and x.shape[2] == 1):
        return int(x.shape[1]), int(x.shape[0])
    raise ValueError(f"components: the mask must be HxW or HxWx1 uint8, got shape {tuple(x.shape)}")


def _connectivity(connectivity):
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or connectivity not in (4, 8):
        raise ValueError(f"components: connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def _area_bounds(min_area, max_area):
    for name, v in (("min_area", min_area), ("max_area", max_area)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise ValueError(f"components: {name} must be an integer, got {v!r}")
    amin = int(min_area)
    amax = C.AREA_NO_LIMIT if max_area is None else int(max_area)
    if amin < 1:
        raise ValueError(f"components: min_area must be at least 1, got {amin}")
    if amax < amin:
        raise ValueError(f"components: max_area {amax} < min_area {amin}")
    return amin, amax


def _device_mask(x, W):
    """A CUDA mask as the pitched HxW view the kernels take (only a row's pixels must be packed)."""
    if x.dtype != torch.uint8:
        raise TypeError("image tensor must be uint8")
    x2 = x[:, :, 0] if x.ndim == 3 else x
    packed = (x2.stride(1) == 1 or W == 1) and (x2.stride(0) >= W or x2.shape[0] == 1)
    return x2 if packed else x2.contiguous()


def _host_mask(x):
    arr = x.numpy() if _is_tensor(x) else np.asarray(x)
    if arr.dtype != np.uint8:
        raise TypeError("image must be uint8")
    return np.ascontiguousarray(arr[:, :, 0] if arr.ndim == 3 else arr)


def _device_label(xc, W, H, conn):
    labels = torch.empty((H, W), dtype=torch.int32, device=xc.device)
    with torch.cuda.device(xc.device):
        stream = torch.cuda.current_stream(xc.device)
        n = _builder(C.components_device, xc.data_ptr(), xc.stride(0) if H > 1 else W, W, H, conn, labels.data_ptr(), W,
                     stream.cuda_stream)
    # keep the input alive until the stream has consumed it
    xc.record_stream(stream)
    return labels, n


def _device_stats(labels, n):
    H, W = labels.shape
    lc = labels if labels.stride(1) == 1 and labels.stride(0) >= W else labels.contiguous()
    table = torch.empty((n + 1, len(STAT_COLUMNS)), dtype=torch.int64, device=labels.device)
    with torch.cuda.device(labels.device):
        stream = torch.cuda.current_stream(labels.device)
        _builder(C.component_stats_device, lc.data_ptr(), lc.stride(0), W, H, n, table.data_ptr(), stream.cuda_stream)
    lc.record_stream(stream)
    return lc, table


def label(x, connectivity: int = 8):
    """Connected components of a mask: (labels, n).

    x: HxW or HxWx1 uint8; a pixel is foreground iff it is != 0.  connectivity 4 (W/E/N/S) or 8 (with the
    diagonals).  labels: int32 HxW, 0 the background, the components numbered 1..n in raster order of their
    first pixel (scipy.ndimage.label's numbering).  A CUDA tensor runs on the k_ccl_* HIP kernels on torch's
    current stream and gives a CUDA tensor (the call synchronises the stream once, to read n); numpy arrays /
    CPU tensors run on the threaded host executor and keep their container.  Bit-identical to
    `label_reference`."""
    W, H = _mask_shape(x)
    conn = _connectivity(connectivity)
    if _is_tensor(x) and x.is_cuda:
        return _device_label(_device_mask(x, W), W, H, conn)
    labels, n = _builder(C.cpu_components, _host_mask(x), conn)
    return (torch.from_numpy(labels) if _is_tensor(x) else labels), n


def label_reference(x, connectivity: int = 8):
    """Golden CPU result of `label`: a raster scan that flood-fills every unlabelled foreground pixel."""
    arr = x.detach().cpu().numpy() if _is_tensor(x) else np.asarray(x)
    _mask_shape(arr)
    return _builder(C.golden_components, _host_mask(arr), _connectivity(connectivity))


def component_stats(labels, n: int):
    """int64 numpy table (n + 1, 7) of the labels 0..n: area, x0, y0, x1, y1, sum_x, sum_y (STAT_COLUMNS).

    Row 0 is the background; x0, y0 inclusive, x1, y1 exclusive; sum_x / area is the centroid.  CUDA labels run
    on k_ccl_stats."""
    if labels.ndim != 2:
        raise ValueError(f"components: labels must be HxW, got shape {tuple(labels.shape)}")
    n = int(n)
    if n < 0:
        raise ValueError(f"components: n must not be negative, got {n}")
    if _is_tensor(labels) and labels.is_cuda:
        if labels.dtype != torch.int32:
            raise TypeError("labels must be int32")
        return _device_stats(labels, n)[1].cpu().numpy()
    arr = labels.numpy() if _is_tensor(labels) else np.asarray(labels)
    if arr.dtype != np.int32:
        raise TypeError("labels must be int32")
    return _builder(C.component_stats, np.ascontiguousarray(arr), n, 0)


def area_filter(x, min_area: int = 1, max_area=None, connectivity: int = 8):
    """Keep the components whose area lies in min_area..max_area (None: no limit); everything else becomes 0.

    The result has the shape, dtype and container of x (kept pixels keep their byte), so it can go back into a
    chain."""
    W, H = _mask_shape(x)
    conn = _connectivity(connectivity)
    amin, amax = _area_bounds(min_area, max_area)
    if _is_tensor(x) and x.is_cuda:
        xc = _device_mask(x, W)
        labels, n = _device_label(xc, W, H, conn)
        labels, table = _device_stats(labels, n)
        out = torch.empty((H, W), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream(x.device)
            _builder(C.area_filter_device, xc.data_ptr(), xc.stride(0) if H > 1 else W, W, H, labels.data_ptr(), W,
                     table.data_ptr(), n, amin, amax, out.data_ptr(), W, stream.cuda_stream)
        # keep the input and the temporaries alive until the stream has consumed them
        for t in (xc, labels, table):
            t.record_stream(stream)
        return out[:, :, None] if x.ndim == 3 else out
    out = _builder(C.cpu_area_filter, _host_mask(x), conn, amin, amax)
    if x.ndim == 3:
        out = out[:, :, None]
    return torch.from_numpy(out) if _is_tensor(x) else out


def remove_small_objects(x, min_area: int, connectivity: int = 8):
    """Drop every component of fewer than min_area pixels."""
    return area_filter(x, min_area, None, connectivity)


def keep_largest(x, connectivity: int = 8):
    """Keep the components of the largest area (all of them on a tie); a frame without foreground stays empty."""
    labels, n = label(x, connectivity)
    if n == 0:
        return area_filter(x, 1, None, connectivity)
    top = int(component_stats(labels, n)[1:, 0].max())
    return area_filter(x, top, None, connectivity)


# ---- distance transform and disc morphology (csrc/include/stripe/distance.h) ----
DISTANCE_NONE = int(C.DISTANCE_NONE)
DISTANCE_OUTPUTS = ("squared", "float", "u8")
_DISTANCE_MODE = {name: k for k, name in enumerate(C.DISTANCE_MODES)}


def _distance_shape(x):
    """(W, H) of a mask HxW or HxWx1 within the side limit; everything else is refused."""
    if x.ndim == 4:
        raise ValueError(f"distance: one frame at a time, got a batch of shape {tuple(x.shape)}")
    if x.ndim == 3 and x.shape[2] == 3:
        raise ValueError("distance: needs a 1-channel image, got C = 3; convert first (gray, threshold, ...)")
    if not (x.ndim == 2 or (x.ndim == 3 and x.shape[2] == 1)):
        raise ValueError(f"distance: the mask must be HxW or HxWx1 uint8, got shape {tuple(x.shape)}")
    W, H = int(x.shape[1]), int(x.shape[0])
    if W < 1 or H < 1:
        raise ValueError(f"distance: empty image ({W}x{H})")
    if W > C.DISTANCE_MAX_SIDE or H > C.DISTANCE_MAX_SIDE:
        raise ValueError(f"distance: {W}x{H} has a side above {C.DISTANCE_MAX_SIDE}")
    return W, H


def _distance_to(to):
    if to not in ("background", "foreground"):
        raise ValueError(f"distance: to must be background or foreground, got {to!r}")
    return to == "foreground"


def _radius(radius):
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise ValueError(f"distance: the radius must be a number, got {radius!r}")
    return int(_builder(C.check_radius, float(radius)))


def _device_distance(xc, W, H, to_fg, mode, t=0):
    """One transform of a device mask on torch's current stream: the int32 plane (squared) or a u8 plane."""
    out = torch.empty((H, W), dtype=torch.int32 if mode == "squared" else torch.uint8, device=xc.device)
    with torch.cuda.device(xc.device):
        stream = torch.cuda.current_stream(xc.device)
        _builder(C.distance_device, xc.data_ptr(), xc.stride(0) if H > 1 else W, W, H, to_fg, _DISTANCE_MODE[mode], t,
                 out.data_ptr(), W, stream.cuda_stream)
    # keep the input alive until the stream has consumed it
    xc.record_stream(stream)
    return out


def distance_transform(x, to: str = "background", output: str = "squared"):
    """Exact Euclidean distance transform of a mask.

    x: HxW or HxWx1 uint8, sides up to 32767; a pixel is foreground iff it is != 0.  to="background"
    (scipy.ndimage.distance_transform_edt's meaning): every pixel gets the distance to the nearest background
    pixel, background pixels get 0; to="foreground" swaps the roles.  The frame edge is not a site.
    output="squared": int32 d^2, DISTANCE_NONE everywhere in a frame without any site; "u8":
    min(255, floor(d)); "float": float32 d (sqrt in float64, rounded; +inf without a site).  The result is HxW.
    A CUDA tensor runs on the k_edt_* HIP kernels on torch's current stream without any synchronisation and
    gives a CUDA tensor; numpy arrays / CPU tensors run on the threaded host executor and keep their container.
    squared and u8 are bit-identical to `distance_transform_reference`."""
    W, H = _distance_shape(x)
    to_fg = _distance_to(to)
    if output not in DISTANCE_OUTPUTS:
        raise ValueError(f"distance: output must be one of {', '.join(DISTANCE_OUTPUTS)}, got {output!r}")
    if _is_tensor(x) and x.is_cuda:
        xc = _device_mask(x, W)
        if output == "u8":
            return _device_distance(xc, W, H, to_fg, "u8")
        d2 = _device_distance(xc, W, H, to_fg, "squared")
        if output == "squared":
            return d2
        d = d2.to(torch.float64).sqrt().to(torch.float32)
        return torch.where(d2 == DISTANCE_NONE, torch.full_like(d, float("inf")), d)
    a = _host_mask(x)
    if output == "u8":
        out = _builder(C.cpu_distance_u8, a, to_fg)
    else:
        out = _builder(C.cpu_distance, a, to_fg)
        if output == "float":
            out = _distance_float(out)
    return torch.from_numpy(out) if _is_tensor(x) else out


def _distance_float(d2):
    d = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    d[d2 == DISTANCE_NONE] = np.inf
    return d


def distance_transform_reference(x, to: str = "background", output: str = "squared"):
    """Golden CPU result of `distance_transform` (numpy): column scans, then the minimum over every column by
    brute force, O(W^2 H); for small frames."""
    arr = x.detach().cpu().numpy() if _is_tensor(x) else np.asarray(x)
    _distance_shape(arr)
    to_fg = _distance_to(to)
    if output not in DISTANCE_OUTPUTS:
        raise ValueError(f"distance: output must be one of {', '.join(DISTANCE_OUTPUTS)}, got {output!r}")
    if output == "u8":
        return _builder(C.golden_distance_u8, _host_mask(arr), to_fg)
    d2 = _builder(C.golden_distance, _host_mask(arr), to_fg)
    return _distance_float(d2) if output == "float" else d2


def _disk_morph(x, op, radius):
    W, H = _distance_shape(x)
    t = _radius(radius)
    if _is_tensor(x) and x.is_cuda:
        xc = _device_mask(x, W)
        out = torch.empty((H, W), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream(x.device)
            _builder(C.disk_morph_device, xc.data_ptr(), xc.stride(0) if H > 1 else W, W, H, op, t, out.data_ptr(), W,
                     stream.cuda_stream)
        xc.record_stream(stream)
        return out[:, :, None] if x.ndim == 3 else out
    out = _builder(C.cpu_disk_morph, _host_mask(x), op, float(radius))
    if x.ndim == 3:
        out = out[:, :, None]
    return torch.from_numpy(out) if _is_tensor(x) else out


def erode_disk(x, radius):
    """Erosion of a mask by the disc {dx^2 + dy^2 <= floor(radius^2)}: 255 where the whole disc lies in the
    foreground (the frame edge does not erode), else 0; any radius >= 0 in a constant number of passes.  Shape and
    container of x; radius 0 binarises."""
    return _disk_morph(x, "erode", radius)


def dilate_disk(x, radius):
    """Dilation by the disc: 255 within radius of a foreground pixel, else 0."""
    return _disk_morph(x, "dilate", radius)


def open_disk(x, radius):
    """dilate_disk(erode_disk(x, radius), radius): removes what is thinner than the disc."""
    return _disk_morph(x, "open", radius)


def close_disk(x, radius):
    """erode_disk(dilate_disk(x, radius), radius): fills what is narrower than the disc."""
    return _disk_morph(x, "close", radius)


# ---- integral images: any-size box filter and local thresholds (csrc/include/stripe/integral.h) ----
WINDOW_OPS = tuple(C.WINDOW_OPS)
WINDOW_MAX_K = int(C.WINDOW_MAX_K)
WINDOW_MAX_K_SQUARES = int(C.WINDOW_MAX_K_SQUARES)
LOCAL_THRESHOLD_METHODS = ("mean", "niblack", "sauvola")
_WINDOW_OP = {name: k for k, name in enumerate(C.WINDOW_OPS)}
_WINDOW_BORDERS = ("reflect101", "replicate", "constant")


def _integral_shape(x):
    """(W, H) of one 1-channel frame HxW or HxWx1 within the side limit; everything else is refused."""
    if x.ndim == 4:
        raise ValueError(f"integral: one frame at a time, got a batch of shape {tuple(x.shape)}")
    if x.ndim == 3 and x.shape[2] == 3:
        raise ValueError("integral: needs a 1-channel image, got C = 3; convert first (gray, threshold, ...)")
    if not (x.ndim == 2 or (x.ndim == 3 and x.shape[2] == 1)):
        raise ValueError(f"integral: the image must be HxW or HxWx1 uint8, got shape {tuple(x.shape)}")
    W, H = int(x.shape[1]), int(x.shape[0])
    if W < 1 or H < 1:
        raise ValueError(f"integral: empty image ({W}x{H})")
    if W > C.INTEGRAL_MAX_SIDE or H > C.INTEGRAL_MAX_SIDE:
        raise ValueError(f"integral: {W}x{H} has a side above {C.INTEGRAL_MAX_SIDE}")
    return W, H


def integral(x, squared: bool = False):
    """The integral image (summed-area table) of a 1-channel frame, OpenCV's layout.

    x: HxW or HxWx1 uint8, sides up to 32767.  The result is (H + 1) x (W + 1) int32 with row 0 and column 0
    zero and I[y][x] the sum of p (of p^2 with squared=True) over y' < y, x' < x, modulo 2^32 like
    cv::integral CV_32S: a rectangle sum below 2^32 is still exact as I[d] - I[b] - I[c] + I[a] in wrapping
    arithmetic.  A CUDA tensor runs on the k_sat_* HIP kernels on torch's current stream without any
    synchronisation and gives a CUDA tensor; numpy arrays / CPU tensors run on the threaded host executor and
    keep their container.  Bit-identical to `integral_reference`."""
    W, H = _integral_shape(x)
    if _is_tensor(x) and x.is_cuda:
        xc = _device_mask(x, W)
        out = torch.empty((H + 1, W + 1), dtype=torch.int32, device=x.device)
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream(x.device)
            _builder(C.integral_device, xc.data_ptr(), xc.stride(0) if H > 1 else W, W, H, bool(squared),
                     out.data_ptr(), W + 1, stream.cuda_stream)
        # keep the input alive until the stream has consumed it
        xc.record_stream(stream)
        return out
    out = _builder(C.cpu_integral, _host_mask(x), bool(squared))
    return torch.from_numpy(out) if _is_tensor(x) else out


def integral_reference(x, squared: bool = False):
    """Golden CPU result of `integral` (numpy): the plain double loop."""
    arr = x.detach().cpu().numpy() if _is_tensor(x) else np.asarray(x)
    _integral_shape(arr)
    return _builder(C.golden_integral, _host_mask(arr), bool(squared))


def _window_args(op, ksize, border, c, k):
    """(op, K, border, c, k) checked the way every layer words it; k is None for the operations without one."""
    if op not in _WINDOW_OP:
        raise ValueError(f"integral: the window operation must be one of {', '.join(WINDOW_OPS)}, got {op!r}")
    if isinstance(ksize, bool) or not isinstance(ksize, (int, np.integer)):
        raise ValueError(f"integral: the window must be an odd integer, got {ksize!r}")
    if border not in _WINDOW_BORDERS:
        raise ValueError(f"integral: the border must be reflect101, replicate or constant, got {border!r}")
    if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
        raise ValueError(f"integral: c must be an integer, got {c!r}")
    if op == "sauvola" and int(c) != 0:
        raise ValueError("integral: sauvola takes no c (its threshold scales the mean); use niblack for an offset")
    if op in ("niblack", "sauvola"):
        k = 0.2 if k is None else float(k)
    elif k is not None:
        raise ValueError(f"integral: {op} takes no k, got {k!r}")
    else:
        k = 0.0
    return op, int(ksize), border, int(c), k


def _check_one_channel(x):
    if (x.ndim == 3 and x.shape[2] == 3) or (x.ndim == 4 and x.shape[3] == 3):
        raise ValueError("integral: needs a 1-channel image, got C = 3; convert first (gray, threshold, ...)")


def _window_stage(x, op, ksize, border, c=0, k=None):
    op, K, border, c, k = _window_args(op, ksize, border, c, k)
    _check_one_channel(x)
    kq = int(_builder(C.window_kq, k))

    def on_device(view, W2, H2, _, stream):
        src, sp, W, H, _c, dst, dp = view
        _builder(C.window_device, src, sp, W, H, _WINDOW_OP[op], K, border, c, kq, dst, dp, stream.cuda_stream)

    return _frame_stage(x, lambda W, H: (W, H, None), on_device,
                        lambda arr, W2, H2, _: _builder(C.cpu_window, arr, op, K, border, c, k))


def box_filter(x, ksize: int, border: str = "reflect101"):
    """The mean over a ksize x ksize window, any odd ksize up to 4095, in a constant number of passes:
    (A + N/2) / N with A the window sum over the frame extended by the border and N = ksize^2 (box3 / box5's
    rule, so ksize 3 and 5 equal `box_blur`).  x: HxW, HxWx1 or a Bx..x1 batch, uint8; the result has x's shape
    and container.  CUDA tensors run on the k_sat_* HIP kernels (integral image, then four table reads per
    pixel) on torch's current stream; numpy arrays / CPU tensors on the host executor; bit-identical to
    `window_reference`."""
    return _window_stage(x, "box", ksize, border)


def local_std(x, ksize: int, border: str = "reflect101"):
    """The local standard deviation over a ksize x ksize window (odd, up to 255): floor(isqrt(N B - A^2) / N)
    with A and B the window sums of p and p^2, at most 127."""
    return _window_stage(x, "std", ksize, border)


def local_threshold(x, ksize: int, method: str = "mean", c: int = 0, k=None, border: str = "reflect101"):
    """A 0 / 255 mask from a threshold that follows the local window (document binarisation).

    method="mean": p > m - c with m the box mean (`adaptive_threshold`'s rule at any odd ksize up to 4095);
    "niblack": p > m + k s - c; "sauvola": p > m (1 + k (s / 128 - 1)), with s the local standard deviation,
    ksize up to 255, k (default 0.2, |k| <= 4) quantised to 1/4096; both in exact integers (the rule:
    stripe/integral.h).  c is an integer in -255..255 and is refused for sauvola."""
    if method not in LOCAL_THRESHOLD_METHODS:
        raise ValueError(f"integral: method must be one of {', '.join(LOCAL_THRESHOLD_METHODS)}, got {method!r}")
    return _window_stage(x, method, ksize, border, c, k)


def window_reference(x, op: str, ksize: int, border: str = "reflect101", c: int = 0, k=None):
    """Golden CPU result of `box_filter` ("box"), `local_std` ("std") and `local_threshold` ("mean", "niblack",
    "sauvola"): the plain loop over the extended frame (numpy)."""
    op, K, border, c, k = _window_args(op, ksize, border, c, k)
    _check_one_channel(x)
    return _reference_frame(x, lambda W, H: lambda arr: _builder(C.golden_window, arr, op, K, border, c, k))


# ---- canny edges and hysteresis thresholding (csrc/include/stripe/canny.h) ----
CANNY_NORMS = tuple(C.CANNY_NORMS)
CANNY_MAX_THRESHOLD = int(C.CANNY_MAX_THRESHOLD)
_CANNY_BORDERS = ("reflect101", "replicate", "constant")


def _canny_shape(x):
    """(W, H) of one 1-channel frame HxW or HxWx1; everything else is refused."""
    if x.ndim == 4:
        raise ValueError(f"canny: one frame at a time, got a batch of shape {tuple(x.shape)}")
    if x.ndim == 3 and x.shape[2] == 3:
        raise ValueError("canny: needs a 1-channel image, got C = 3; convert first (gray, threshold, ...)")
    if not (x.ndim == 2 or (x.ndim == 3 and x.shape[2] == 1)):
        raise ValueError(f"canny: the image must be HxW or HxWx1 uint8, got shape {tuple(x.shape)}")
    W, H = int(x.shape[1]), int(x.shape[0])
    if W < 1 or H < 1:
        raise ValueError(f"canny: empty image ({W}x{H})")
    if W * H > 2 ** 31 - 2:
        raise ValueError(f"canny: {W}x{H} pixels exceed 2^31 - 2")
    return W, H


def _thresholds(low, high, limit):
    """(low, high) as ints: any Python or numpy number whose value is integral, 0 <= low <= high <= limit."""
    vals = []
    for v in (low, high):
        ok = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))
        if ok and isinstance(v, (float, np.floating)):
            ok = bool(np.isfinite(v)) and float(v) == int(v)
        vals.append(int(v) if ok else None)
    if None in vals or not 0 <= vals[0] <= vals[1] <= limit:
        raise ValueError(f"canny: the thresholds must be integers with 0 <= low <= high <= {limit}, "
                         f"got low = {low!r}, high = {high!r}")
    return vals[0], vals[1]


def _canny_args(low, high, norm, border):
    low, high = _thresholds(low, high, CANNY_MAX_THRESHOLD)
    if norm not in CANNY_NORMS:
        raise ValueError(f"canny: the norm must be l1 or l2, got {norm!r}")
    if border not in _CANNY_BORDERS:
        raise ValueError(f"canny: the border must be reflect101, replicate or constant, got {border!r}")
    return low, high, norm, border


def _edge_stage(x, W, H, device_call, host_call):
    """One 1-channel frame through a C.*_device call (src, src_pitch, W, H, ..., dst, dst_pitch, stream) on torch's
    current stream, or through the host executor; the u8 result has x's shape and container."""
    if _is_tensor(x) and x.is_cuda:
        xc = _device_mask(x, W)
        out = torch.empty((H, W), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream(x.device)
            device_call(xc.data_ptr(), xc.stride(0) if H > 1 else W, out.data_ptr(), W, stream.cuda_stream)
        # keep the input alive until the stream has consumed it
        xc.record_stream(stream)
        return out[:, :, None] if x.ndim == 3 else out
    out = host_call(_host_mask(x))
    if x.ndim == 3:
        out = out[:, :, None]
    return torch.from_numpy(out) if _is_tensor(x) else out


def canny(x, low, high, norm: str = "l1", border: str = "reflect101"):
    """Canny edge detection: a u8 edge map, 255 on an edge, 0 elsewhere.

    x: HxW or HxWx1 uint8.  The Sobel gradient (Gx, Gy; the frame extended by `border`: reflect101, replicate or
    constant) gives the magnitude |Gx| + |Gy| (norm="l1", at most 2040) or Gx^2 + Gy^2 (norm="l2", compared with
    low^2 and high^2; no root is taken); a pixel survives non-maximum suppression against its two neighbours
    along the gradient (four sectors, integers only; of a two-pixel plateau exactly one pixel survives);
    survivors above `high` are strong, those above `low` weak, and a weak pixel is kept iff it is 8-connected
    through survivors to a strong one.  low, high: integers (any Python or numpy number whose value is
    integral) with 0 <= low <= high <= 2040.  No blur is built in: chain `gaussian_blur` in front.  The rule:
    stripe/canny.h.  A CUDA tensor runs on the k_canny_* HIP kernels and the union-find forest of k_ccl_* on
    torch's current stream and gives a CUDA tensor (the call synchronises the stream once); numpy arrays / CPU
    tensors run on the threaded host executor and keep their container.  Bit-identical to `canny_reference`."""
    W, H = _canny_shape(x)
    low, high, norm, border = _canny_args(low, high, norm, border)
    return _edge_stage(
        x, W, H,
        lambda src, sp, dst, dp, s: _builder(C.canny_device, src, sp, W, H, low, high, norm, border, dst, dp, s),
        lambda a: _builder(C.cpu_canny, a, low, high, norm, border))


def canny_classes(x, low, high, norm: str = "l1", border: str = "reflect101"):
    """The class plane of `canny` before the hysteresis, u8: 2 a strong pixel (it survives the suppression and its
    magnitude is above high), 1 a weak one (above low), 0 everything else.  On a CUDA tensor the call queues
    k_canny_nms and does not synchronise."""
    W, H = _canny_shape(x)
    low, high, norm, border = _canny_args(low, high, norm, border)
    return _edge_stage(
        x, W, H,
        lambda src, sp, dst, dp, s: _builder(C.canny_classes_device, src, sp, W, H, low, high, norm, border, dst, dp, s),
        lambda a: _builder(C.cpu_canny_classes, a, low, high, norm, border))


def canny_reference(x, low, high, norm: str = "l1", border: str = "reflect101"):
    """Golden CPU result of `canny` (numpy): plain loops over the extended frame, then a flood fill from every
    strong pixel."""
    arr = x.detach().cpu().numpy() if _is_tensor(x) else np.asarray(x)
    _canny_shape(arr)
    low, high, norm, border = _canny_args(low, high, norm, border)
    return _builder(C.golden_canny, _host_mask(arr), low, high, norm, border)


def hysteresis_threshold(x, low, high, connectivity: int = 8):
    """Hysteresis thresholding of a 1-channel frame: a u8 mask, 255 where p > low and the pixel is connected,
    through pixels with p > low (connectivity 4 or 8), to a pixel with p > high; 0 elsewhere.  low, high:
    integers with 0 <= low <= high <= 255.  Useful on `sobel` output or on `distance_transform(..., "u8")`.
    Containers and streams as `canny`; bit-identical to `hysteresis_threshold_reference`."""
    W, H = _canny_shape(x)
    low, high = _thresholds(low, high, int(C.HYSTERESIS_MAX_THRESHOLD))
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or connectivity not in (4, 8):
        raise ValueError(f"canny: connectivity must be 4 or 8, got {connectivity!r}")
    conn = int(connectivity)
    return _edge_stage(
        x, W, H,
        lambda src, sp, dst, dp, s: _builder(C.hysteresis_device, src, sp, W, H, low, high, conn, dst, dp, s),
        lambda a: _builder(C.cpu_hysteresis_threshold, a, low, high, conn))


def hysteresis_threshold_reference(x, low, high, connectivity: int = 8):
    """Golden CPU result of `hysteresis_threshold` (numpy): a flood fill from every pixel above high."""
    arr = x.detach().cpu().numpy() if _is_tensor(x) else np.asarray(x)
    _canny_shape(arr)
    low, high = _thresholds(low, high, int(C.HYSTERESIS_MAX_THRESHOLD))
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or connectivity not in (4, 8):
        raise ValueError(f"canny: connectivity must be 4 or 8, got {connectivity!r}")
    return _builder(C.golden_hysteresis_threshold, _host_mask(arr), low, high, int(connectivity))


def clear_cache() -> None:
    with _cache_lock:
        _engines.clear()
    C.distance_release_scratch()
    C.integral_release_scratch()
    C.canny_release_scratch()


__all__ = [
    "FILTERS", "apply", "reference", "grayscale", "contrast", "invert", "brightness", "threshold",
    "gaussian_blur", "box_blur", "sobel", "sharpen", "laplace", "emboss",
    "median", "bilateral", "erode", "dilate", "morph_open", "morph_close", "conv2d", "sep_conv2d", "large_blur", "clear_cache",
    "color_matrix", "sepia", "saturation", "swap_rb", "rgb_to_ycbcr", "ycbcr_to_rgb",
    "histogram", "equalize", "autocontrast", "threshold_otsu", "otsu_level",
    "unsharp_mask", "morph_gradient", "top_hat", "black_hat", "adaptive_threshold",
    "combine", "absdiff", "add", "subtract", "blend", "minimum", "maximum",
    "resize", "resize_reference", "RESIZE_MODES",
    "orient", "orient_reference", "flip", "rot90", "transpose_image", "crop", "exif_orientation", "ORIENTATIONS",
    "warp_affine", "rotate", "warp_reference", "WARP_MODES", "WARP_BORDERS",
    "warp_perspective", "perspective_from_points", "rectify_quad", "undistort", "remap", "mesh_warp",
    "remap_reference", "MESH_SPACINGS",
    "label", "label_reference", "component_stats", "area_filter", "remove_small_objects", "keep_largest",
    "STAT_COLUMNS",
    "distance_transform", "distance_transform_reference", "erode_disk", "dilate_disk", "open_disk", "close_disk",
    "DISTANCE_NONE", "DISTANCE_OUTPUTS",
    "integral", "integral_reference", "box_filter", "local_std", "local_threshold", "window_reference",
    "WINDOW_OPS", "WINDOW_MAX_K", "WINDOW_MAX_K_SQUARES", "LOCAL_THRESHOLD_METHODS",
    "canny", "canny_reference", "canny_classes", "hysteresis_threshold", "hysteresis_threshold_reference",
    "CANNY_NORMS", "CANNY_MAX_THRESHOLD",
]
