"""starcop_amd.stacks, the image-stack front-end of the mask / label-image operators, on CPU tensors: no device involved."""
import numpy as np
import pytest
import torch

from starcop_amd import stacks


def test_read_back_keeps_bytes_dtype_and_shape():
    f32 = np.array([[0x7fc01234, 0x80000000, 0x7f800000]], dtype=np.uint32).view(np.float32)      # NaN with a payload, -0.0, inf
    cols = {"i32": torch.arange(6, dtype=torch.int32).reshape(1, 2, 3) - 3,
            "f64": torch.tensor([[1.5, -2.0 ** -1060], [float("nan"), 1e300]], dtype=torch.float64),
            "i64": torch.zeros((1, 0), dtype=torch.int64),
            "f32": torch.from_numpy(f32.copy())}
    got = stacks.read_back(cols)
    assert list(got) == list(cols)
    for f, t in cols.items():
        want = t.numpy()
        assert got[f].dtype == want.dtype and got[f].shape == want.shape, f
        assert got[f].tobytes() == want.tobytes(), f
        assert got[f].flags.c_contiguous and got[f].flags.aligned, f
        assert not np.shares_memory(got[f], want) and not any(np.shares_memory(got[f], got[g]) for g in cols if g != f), f
    assert got["f32"].view(np.uint32).tolist() == [[0x7fc01234, 0x80000000, 0x7f800000]]
    assert stacks.read_back({}) == {}
    # a column that is a strided view, and keys that are tuples
    x = torch.arange(24, dtype=torch.int64).reshape(2, 3, 4)
    got = stacks.read_back({("a", 0): x[:, :, 1], ("a", 1): x[1]})
    assert np.array_equal(got["a", 0], x[:, :, 1].numpy()) and np.array_equal(got["a", 1], x[1].numpy())


def test_stack3_shape_check():
    for bad in (np.zeros(5), torch.zeros((1, 2, 3, 4))):
        with pytest.raises(ValueError, match=r"some_call: expected an \(H, W\) or \(N, H, W\) mask, got"):
            stacks.stack3(bad, "some_call", "mask")
    with pytest.raises(ValueError, match="some_call: expected a numpy array or a tensor, got list"):
        stacks.stack3([[0, 1]], "some_call")
    a, t = np.zeros((4, 5)), torch.zeros((2, 4, 5))
    assert stacks.check_stack(a, "t") is True and stacks.check_stack(t, "t") is False       # the check alone: no view is made
    with pytest.raises(ValueError, match=r"some_call: expected an \(H, W\) or \(N, H, W\) label image, got \(5,\)"):
        stacks.check_stack(torch.zeros(5), "some_call", "label image")
    x3, single = stacks.stack3(a, "t")
    assert single and x3.shape == (1, 4, 5) and np.shares_memory(x3, a)
    x3, single = stacks.stack3(t, "t")
    assert not single and x3 is t
    with pytest.raises(ValueError, match="t: plane 1 has shape"):
        stacks.stack_like(torch.zeros((4, 6)), (1, 4, 5), "t: plane 1")
    with pytest.raises(ValueError, match="t: plane 1 must be a device tensor, got ndarray"):
        stacks.stack_like(np.zeros((4, 5)), (1, 4, 5), "t: plane 1")
    with pytest.raises(ValueError, match=r"t: plane 1: expected an \(H, W\) or \(N, H, W\) array"):
        stacks.stack_like(torch.zeros(5), (1, 4, 5), "t: plane 1")
    assert stacks.stack_like(torch.zeros((4, 5)), torch.Size((1, 4, 5)), "t: plane 1").shape == (1, 4, 5)


def test_counts_front_end():
    c = stacks.counts_i32(7, 1, "cpu", "t")
    assert c.dtype == torch.int32 and c.tolist() == [7]
    c = stacks.counts_i32(torch.tensor([3, 0, 9], dtype=torch.int64), 3, "cpu", "t")
    assert c.dtype == torch.int32 and c.tolist() == [3, 0, 9] and c.is_contiguous()
    assert stacks.counts_i32(np.array([[2], [5]]), 2, None, "t").tolist() == [2, 5]
    for counts, N in ((4, 2), (torch.zeros(2, dtype=torch.int32), 1), (torch.zeros(0, dtype=torch.int32), 1)):
        with pytest.raises(ValueError, match=r"some_call: \d counts for \d images"):
            stacks.counts_i32(counts, N, "cpu", "some_call")


def test_plane_operand_reads_dense_planes_in_place():
    N, H, W = 2, 5, 7
    x = torch.arange(N * 4 * H * W, dtype=torch.float32).reshape(N, 4, H, W)
    t, stride = stacks.plane_operand(x[:, 2], torch.float32)
    assert t.data_ptr() == x[:, 2].data_ptr() and stride == 4 * H * W
    t, stride = stacks.plane_operand(x[:, 2])                       # any dtype, as it is
    assert t.data_ptr() == x[:, 2].data_ptr() and stride == 4 * H * W
    y = torch.arange(N * W * H, dtype=torch.float32).reshape(N, W, H).transpose(1, 2)
    t, stride = stacks.plane_operand(y, torch.float32)
    assert t.data_ptr() != y.data_ptr() and t.is_contiguous() and stride == H * W and torch.equal(t, y)
    t, stride = stacks.plane_operand(x[:1, 1], torch.float32)       # one image: the stride is never used, H * W by convention
    assert t.data_ptr() == x[:1, 1].data_ptr() and stride == H * W
    # conversion: to uint8 as x != 0, to float32 by value
    m, stride = stacks.plane_operand(torch.tensor([[[0.0, 0.25], [-3.0, float("nan")]]]), torch.uint8)
    assert m.dtype == torch.uint8 and m.tolist() == [[[0, 1], [1, 1]]] and stride == 4
    f, _ = stacks.plane_operand(torch.tensor([[[1, 2], [3, 4]]], dtype=torch.int16), torch.float32)
    assert f.dtype == torch.float32 and f.tolist() == [[[1.0, 2.0], [3.0, 4.0]]]


def test_finish_and_output_columns():
    import ctypes as C

    class Args(C.Structure):
        _fields_ = [("a", C.c_void_p), ("b", C.c_void_p)]
    args = Args()
    out = stacks.output_columns(args, [("a", torch.int64, (2, 3)), ("b", torch.float32, (2, 0, 4))], "cpu")
    assert out["a"].shape == (2, 3) and out["a"].dtype == torch.int64 and out["b"].shape == (2, 0, 4) and out["b"].dtype == torch.float32
    assert args.a == out["a"].data_ptr() and args.b is None           # NULL for the column without elements
    t = torch.arange(6).reshape(1, 2, 3)
    assert stacks.finish(t, False, False) is t and stacks.finish(t, True, False).shape == (2, 3)
    h = stacks.finish(t, True, True)
    assert isinstance(h, np.ndarray) and h.tolist() == [[0, 1, 2], [3, 4, 5]]
