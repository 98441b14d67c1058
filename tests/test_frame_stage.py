"""The frame driver of the whole-frame stages (`ops._frame_stage`): what resize, orient, warp and remap
promise about containers, ranks, batches, views and streams, on one fixed small request each.  The kernels and
rules have their own tests (test_resize.py, test_gpu_resize.py, ...); the frames here are 37x53 and 64x65
pixels, one below and one just over a tile side."""
import re

import numpy as np
import pytest

import mpi_cuda_imagemanipulation_amd as m

ops, C = m.ops, m._C
torch = pytest.importorskip("torch")

SIZES = ((37, 53), (64, 65))  # (W, H)
PERSPECTIVE = [1.02, 0.05, -1.5, -0.03, 0.98, 2.0, 0.0004, -0.0002, 1.0]


def _rotation(W, H):
    minv, W2, H2 = C.rotate_matrix(30.0, False, W, H)
    return np.asarray(minv).reshape(2, 3), (H2, W2)


def _mesh(W, H):
    mesh, spacing = C.perspective_mesh(PERSPECTIVE, False, W, H, W, H, 8)
    assert spacing == 8
    return mesh


class Stage:
    """run(x, W, H) and reference(x, W, H) of one request; shape(W, H) is the result's (H2, W2)."""

    def __init__(self, run, reference, shape, pitched=True):
        self.run, self.reference, self.shape, self.pitched = run, reference, shape, pitched


STAGES = {
    "resize": Stage(lambda x, W, H: ops.resize(x, size=(30, 20), mode="bilinear"),
                    lambda x, W, H: ops.resize_reference(x, size=(30, 20), mode="bilinear"),
                    lambda W, H: (30, 20), pitched=False),
    "orient": Stage(lambda x, W, H: ops.orient(x, "rot90", (3, 2, 11, 9)),
                    lambda x, W, H: ops.orient_reference(x, "rot90", (3, 2, 11, 9)),
                    lambda W, H: (9, 11)),
    "rotate": Stage(lambda x, W, H: ops.rotate(x, 30.0, expand=False),
                    lambda x, W, H: ops.warp_reference(x, _rotation(W, H)[0], size=_rotation(W, H)[1], inverse=True),
                    lambda W, H: (H, W)),
    "mesh": Stage(lambda x, W, H: ops.mesh_warp(x, _mesh(W, H), 8),
                  lambda x, W, H: ops.remap_reference(x, _mesh(W, H), 8),
                  lambda W, H: (H, W)),
}
stages = pytest.mark.parametrize("stage", list(STAGES.values()), ids=list(STAGES))
sizes = pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")


def frame(W, H, *tail):
    return np.random.default_rng(W * 7919 + H * 31 + len(tail)).integers(0, 256, (H, W) + tail, dtype=np.uint8)


@stages
@sizes
def test_numpy_input_keeps_its_rank(stage, size):
    W, H = size
    for tail in ((), (1,), (3,)):
        a = frame(W, H, *tail)
        got = stage.run(a, W, H)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8
        assert got.shape == stage.shape(W, H) + tail
        assert (got == stage.reference(a, W, H)).all()
    # HxWx1 is the gray frame with one more axis
    a = frame(W, H)
    assert (stage.run(a[:, :, None], W, H)[:, :, 0] == stage.run(a, W, H)).all()


@stages
@sizes
def test_cpu_tensor_gives_a_cpu_tensor(stage, size):
    W, H = size
    for tail in ((), (1,), (3,)):
        a = frame(W, H, *tail)
        got = stage.run(torch.from_numpy(a), W, H)
        assert isinstance(got, torch.Tensor) and not got.is_cuda and got.dtype == torch.uint8
        assert (got.numpy() == stage.reference(a, W, H)).all()


@stages
@sizes
def test_batch_equals_the_frames_stacked(stage, size):
    W, H = size
    a = np.stack([frame(W, H, 3), frame(W, H, 3)[::-1].copy()])
    ref = np.stack([stage.reference(a[0], W, H), stage.reference(a[1], W, H)])
    got = stage.run(a, W, H)
    assert isinstance(got, np.ndarray) and (got == ref).all()
    got = stage.run(torch.from_numpy(a), W, H)
    assert isinstance(got, torch.Tensor) and (got.numpy() == ref).all()


@stages
@sizes
def test_empty_batch(stage, size):
    W, H = size
    for ch in (1, 3):
        want = (0,) + stage.shape(W, H) + (ch,)
        got = stage.run(np.empty((0, H, W, ch), np.uint8), W, H)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want
        got = stage.run(torch.empty((0, H, W, ch), dtype=torch.uint8), W, H)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and tuple(got.shape) == want


@stages
def test_refusals(stage):
    W, H = SIZES[0]
    for x in (np.zeros((2, H, W, 2), np.uint8), torch.zeros((2, H, W, 2), dtype=torch.uint8),
              np.zeros((0, H, W, 2), np.uint8)):
        text = f"a batch must be BxHxWxC with C in (1, 3), got {tuple(x.shape)}"
        with pytest.raises(ValueError, match=re.escape(text)):
            stage.run(x, W, H)
    with pytest.raises(ValueError, match=re.escape(f"image must be HxW or HxWx3 uint8, got shape ({H}, {W}, 2)")):
        stage.run(np.zeros((H, W, 2), np.uint8), W, H)
    for x in (np.zeros((H, W), np.float32), np.zeros((H, W, 3), np.int16), torch.zeros((H, W), dtype=torch.float32),
              np.zeros((2, H, W, 3), np.float32)):
        with pytest.raises(TypeError, match="image must be uint8"):
            stage.run(x, W, H)


# ---- on the GPU: one small launch per case ----
def _count_copies(monkeypatch):
    """The dtypes of the tensors whose .contiguous() is called from here on."""
    calls, real = [], torch.Tensor.contiguous

    def contiguous(self, *args, **kwargs):
        calls.append(self.dtype)
        return real(self, *args, **kwargs)
    monkeypatch.setattr(torch.Tensor, "contiguous", contiguous)
    return calls


@pytest.mark.gpu
@stages
@sizes
def test_gpu_contiguous_tensor(stage, size):
    W, H = size
    for tail in ((), (1,), (3,)):
        a = frame(W, H, *tail)
        got = stage.run(torch.from_numpy(a).cuda(), W, H)
        assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous()
        assert tuple(got.shape) == stage.shape(W, H) + tail
        assert (got.cpu().numpy() == stage.reference(a, W, H)).all()
    with pytest.raises(TypeError, match="image tensor must be uint8"):
        stage.run(torch.zeros((H, W), dtype=torch.float32, device="cuda"), W, H)


@pytest.mark.gpu
@stages
@sizes
def test_gpu_row_pitched_view_is_read_in_place(stage, size, monkeypatch):
    W, H = size
    for tail in ((), (3,)):
        base = torch.from_numpy(frame(W + 9, H, *tail)).cuda()
        x = base[:, 5:5 + W]
        assert not x.is_contiguous()
        ref = stage.reference(x.cpu().numpy(), W, H)
        calls = _count_copies(monkeypatch)
        got = stage.run(x, W, H)
        monkeypatch.undo()
        assert (got.cpu().numpy() == ref).all()
        if stage.pitched:  # (resize copies every view)
            assert torch.uint8 not in calls


@pytest.mark.gpu
@stages
@sizes
def test_gpu_view_with_strided_pixels_is_copied(stage, size, monkeypatch):
    W, H = size
    for tail in ((), (3,)):
        x = torch.from_numpy(frame(2 * W, H, *tail)).cuda()[:, ::2]
        ref = stage.reference(x.cpu().numpy(), W, H)
        calls = _count_copies(monkeypatch)
        got = stage.run(x, W, H)
        monkeypatch.undo()
        assert calls.count(torch.uint8) == 1
        assert (got.cpu().numpy() == ref).all()


@pytest.mark.gpu
@stages
@sizes
def test_gpu_batch(stage, size):
    W, H = size
    a = np.stack([frame(W, H, 3), frame(W, H, 3)[::-1].copy()])
    got = stage.run(torch.from_numpy(a).cuda(), W, H)
    assert got.is_cuda and tuple(got.shape) == (2,) + stage.shape(W, H) + (3,)
    assert (got.cpu().numpy() == np.stack([stage.reference(a[0], W, H), stage.reference(a[1], W, H)])).all()
    empty = stage.run(torch.empty((0, H, W, 3), dtype=torch.uint8, device="cuda"), W, H)
    assert empty.is_cuda and tuple(empty.shape) == (0,) + stage.shape(W, H) + (3,)


@pytest.mark.gpu
@stages
@sizes
def test_gpu_second_stream(stage, size):
    W, H = size
    a = frame(W, H, 3)
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        x = torch.from_numpy(a).cuda()
        got = stage.run(x, W, H)
    other.synchronize()
    assert (got.cpu().numpy() == stage.reference(a, W, H)).all()
