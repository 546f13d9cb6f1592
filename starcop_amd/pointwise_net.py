"""The pointwise regression networks of the reference on the HIP kernels of csrc/pwreg.hip.

Mirrors starcop/models/architectures/baselines.py:
  SimpleCNN_v2 :43-53 (one 1x1 convolution), SimpleCNN_v3 :56-70 (two, input -> input -> output, no activation between).
``state_dict`` keys and shapes are the reference's (``cnn_layers.{0,1}.{weight,bias}``); the ``torch.nn.Conv2d`` members only hold
the parameters -- the forward is ``sc_pwreg_fwd``, the backward one ``sc_pwreg_train_sweep`` + ``sc_pwreg_finalize`` over the
incoming gradient.  The parameters live in one flat fp32 buffer in ``state_dict`` order, which is both what the kernels read and
what :class:`starcop_amd.optim.FusedAdam` steps.  There is no input gradient and no torch fallback.
"""
import torch

from . import _lib
from ._lib import check, ptr, stream


def _check_channels(name, c):
    if not isinstance(c, int) or not 1 <= c <= _lib.PWREG_MAXC:
        raise ValueError(f"{name} must be an integer in 1..{_lib.PWREG_MAXC} (one MFMA tile), got {c!r}")


class _PointwiseNet(torch.nn.Module):
    layers = 1
    range_check_every = 0          # FusedAdam's periodic fp16-split range check: nothing here is split

    def __init__(self, input_channel_size=13, output_channel_size=12):
        super().__init__()
        _check_channels("input_channel_size", input_channel_size)
        _check_channels("output_channel_size", output_channel_size)
        self.cin, self.cout = input_channel_size, output_channel_size
        self.c1 = input_channel_size if self.layers == 2 else output_channel_size
        convs = [torch.nn.Conv2d(in_channels=self.cin, out_channels=self.c1, kernel_size=1, stride=1)]
        if self.layers == 2:
            convs.append(torch.nn.Conv2d(in_channels=self.c1, out_channels=self.cout, kernel_size=1, stride=1))
        self.cnn_layers = torch.nn.Sequential(*convs)
        self._pflat = self._gflat = None
        self._part = None

    def _dims(self):
        return self.cin, self.c1, self.cout, self.layers

    # -- the flat-storage protocol of FusedAdam (see HyperStarcopUNet) ----------------------------
    def _ensure_flat(self):
        params = list(self.parameters())
        dev = params[0].device
        ok = self._pflat is not None and self._pflat.device == dev
        if ok:
            off, base = 0, self._pflat.data_ptr()
            for p in params:
                if p.data_ptr() != base + 4 * off or p.dtype != torch.float32:
                    ok = False
                    break
                off += p.numel()
        if not ok:
            total = sum(p.numel() for p in params)
            flat = torch.empty(total, dtype=torch.float32, device=dev)
            off = 0
            for p in params:
                n = p.numel()
                flat[off:off + n].copy_(p.data.reshape(-1).float())
                p.data = flat[off:off + n].view(p.shape)
                off += n
            self._pflat = flat
            self._gflat = torch.zeros(total, dtype=torch.float32, device=dev)
            self._part = None
        return params

    def flat_parameters(self):
        self._ensure_flat()
        return self._pflat

    def flat_grads(self):
        self._ensure_flat()
        return self._gflat

    def _grad_view(self, p):
        off = (p.data_ptr() - self._pflat.data_ptr()) // 4
        return self._gflat[off:off + p.numel()].view(p.shape)

    def mark_parameters_changed(self):
        """The kernels read the flat buffer directly: nothing is cached."""

    def check_split_range(self, sync_ranks=False):
        return True

    # -- kernels -----------------------------------------------------------------------------------
    def _checked_input(self, x, channels, what):
        _lib.require_device(x)
        if x.dim() != 4 or x.shape[1] != channels:
            raise ValueError(f"{type(self).__name__}: {what} must be (N, {channels}, H, W), got {tuple(x.shape)}")
        return x.contiguous().float()

    def _forward_impl(self, x):
        lib = _lib.load()
        x = self._checked_input(x, self.cin, "x")
        N, _, H, W = x.shape
        pred = torch.empty((N, self.cout, H, W), dtype=torch.float32, device=x.device)
        check(lib.sc_pwreg_fwd(ptr(x), ptr(self.flat_parameters()), N, *self._dims(), H, W, ptr(pred), stream()))
        return pred

    def sweep_gradients(self, x, y_or_g, mode, loss_sum=None):
        """``sc_pwreg_train_sweep`` + ``sc_pwreg_finalize`` into the flat gradient buffer.  ``mode`` is ``_lib.REG_L1`` / ``REG_MSE``
        (``y_or_g`` is the target; ``loss_sum``, a one-element float64 device tensor, receives sum |d| or sum d^2) or
        ``_lib.PWREG_G_FROM_MEMORY`` (``y_or_g`` is dL/dpred).  Returns the number of elements n of the prediction."""
        lib = _lib.load()
        x = self._checked_input(x, self.cin, "x")
        t = self._checked_input(y_or_g, self.cout, "the target" if mode != _lib.PWREG_G_FROM_MEMORY else "the gradient")
        if t.shape[0] != x.shape[0] or t.shape[2:] != x.shape[2:]:
            raise ValueError(f"{type(self).__name__}: x {tuple(x.shape)} and target {tuple(t.shape)} do not match")
        N, _, H, W = x.shape
        flat, grad = self.flat_parameters(), self.flat_grads()
        nb = lib.sc_pwreg_sweep_blocks(N, H, W)
        if self._part is None or self._part.numel() < nb * _lib.PWREG_PART_DOUBLES or self._part.device != x.device:
            self._part = torch.empty(nb * _lib.PWREG_PART_DOUBLES, dtype=torch.float64, device=x.device)
        n = t.numel()
        scale = {_lib.REG_L1: 1.0 / n, _lib.REG_MSE: 2.0 / n, _lib.PWREG_G_FROM_MEMORY: 1.0}[mode]
        st = stream()
        check(lib.sc_pwreg_train_sweep(ptr(x), ptr(t), ptr(flat), N, *self._dims(), H, W, mode, ptr(self._part), st))
        check(lib.sc_pwreg_finalize(ptr(self._part), nb, ptr(flat), *self._dims(), scale, ptr(grad), ptr(loss_sum), st))
        return n

    def forward(self, x):
        """(N, Cin, H, W) -> (N, Cout, H, W), fp32."""
        _lib.require_device(x)
        if x.requires_grad:
            raise RuntimeError(f"{type(self).__name__} has no input gradient: pass an input that does not require grad")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return _PointwiseFunction.apply(self, x, *self._ensure_flat())
        return self._forward_impl(x)


class _PointwiseFunction(torch.autograd.Function):
    """Whole-network autograd node: backward is the moment sweep over the incoming gradient, into the flat gradient buffer."""

    @staticmethod
    def forward(ctx, net, x, *params):
        ctx.net = net
        ctx.save_for_backward(x)
        return net._forward_impl(x)

    @staticmethod
    def backward(ctx, g):
        net = ctx.net
        (x,) = ctx.saved_tensors
        params = net._ensure_flat()
        # a p.grad kept from the last backward is a view of the flat gradient buffer, which the finalize overwrites: move it onto a
        # snapshot and hand autograd a copy, so that accumulation computes old + new (as HyperStarcopUNet does)
        aliased = [p.grad is not None and p.grad.data_ptr() == net._grad_view(p).data_ptr() for p in params]
        if any(aliased):
            snap = net._gflat.clone()
            base = net._gflat.data_ptr()
            for p, al in zip(params, aliased):
                if al:
                    off = (p.grad.data_ptr() - base) // 4
                    p.grad = snap[off:off + p.numel()].view(p.shape)
        net.sweep_gradients(x, g, _lib.PWREG_G_FROM_MEMORY)
        grads = [net._grad_view(p).clone() if al else net._grad_view(p) for p, al in zip(params, aliased)]
        return (None, None) + tuple(gr if p.requires_grad else None for gr, p in zip(grads, params))


class SimpleCNN_v2(_PointwiseNet):
    """``Conv2d(input_channel_size, output_channel_size, 1)`` (baselines.py:43-53)."""
    layers = 1


class SimpleCNN_v3(_PointwiseNet):
    """``Conv2d(in, in, 1)`` then ``Conv2d(in, out, 1)`` with nothing between them (baselines.py:56-70)."""
    layers = 2
