"""sha256 of the logits and of every gradient of one training step on a fixed batch, and of the logits of the eval-mode forward that
follows it (the inference path, on the running statistics that step left): run it under two builds of the library
(STARCOP_HIP_LIB=...) or two versions of the package to show that a change is bit-neutral.
python tools/step_digest.py [--size 256] [--batch 4] [--precision fp32] [--launches FILE]

--launches FILE also writes one line per library call of the step and the eval forward, so that two versions of the package can be
compared launch by launch (diff): the symbol, every scalar argument, every scalar field of a struct passed by reference, and each
pointer as the index of its first appearance in the log (aliasing is compared, addresses are not); a stream handle reads "main" or
"side".  Host queries -- calls without any pointer argument, which can neither launch nor touch memory -- are not logged."""
import sys, os, argparse, hashlib
import ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class LaunchLog:
    """recording proxy for starcop_amd._lib._lib: every attribute is the library's, calls with a pointer argument are logged first"""

    def __init__(self, lib, signatures, out, streams):
        self._lib, self._sig, self._out, self._streams, self._ptrs = lib, signatures, out, streams, {}

    def _ptr(self, v):
        v = v.value if isinstance(v, C.c_void_p) else v
        return "null" if not v else "p%d" % self._ptrs.setdefault(int(v), len(self._ptrs))

    def _value(self, v, ty=None):
        if ty is C.c_void_p or isinstance(v, C.c_void_p) or v is None:
            return self._ptr(v)
        if hasattr(v, "_obj"):                  # byref(struct)
            return self._value(v._obj)
        if isinstance(v, C.Structure):
            return "{" + " ".join(f"{n}={self._value(getattr(v, n), t)}" for n, t in v._fields_) + "}"
        if isinstance(v, C.Array):
            return "[" + " ".join(self._value(e, v._type_) for e in v) + "]"
        return repr(v.value if hasattr(v, "value") else v)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        types = self._sig.get(name, (None, []))[1]
        if not any(t is C.c_void_p or issubclass(t, C._Pointer) for t in types):
            return fn

        def call(*args):
            names = {int(h or 0): s for s, h in self._streams().items()}
            vals = []
            for k, (v, t) in enumerate(zip(args, types)):
                if t is C.c_void_p and (name == "sc_stream_wait_stream" or k == len(types) - 1):
                    h = int((v.value if isinstance(v, C.c_void_p) else v) or 0)
                    vals.append(names.get(h, "stream?"))
                else:
                    vals.append(self._value(v, t))
            self._out.write(name + " " + " ".join(vals) + "\n")
            return fn(*args)
        setattr(self, name, call)       # (one object per symbol, like ctypes: callers may compare entry points with `is`)
        return call


def main():
    import torch
    from bench import synth_batch
    from starcop_amd import _lib, model_module as mm
    ap = argparse.ArgumentParser(); ap.add_argument("--size", type=int, default=256); ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--precision", default="fp32"); ap.add_argument("--launches", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = mm.ModelModule(mm.default_settings(pos_weight=1, precision=a.precision)).to(dev).train()
    batch = synth_batch(a.batch, a.size, a.size, 1, dev)
    net = model.network
    log = None
    if a.launches:
        log = open(a.launches, "w")
        _lib._lib = LaunchLog(_lib.load(), _lib.SIGNATURES, log, lambda: {
            "side": net._side_stream.cuda_stream if net._side_stream is not None else -1, "main": torch.cuda.current_stream().cuda_stream})
    model.zero_grad()
    loss = model.training_step(batch, 0)
    # (the gradient that autograd hands to the backward walk is a temporary of the caller: take the cached free blocks of its size first,
    # so that it gets an address of its own and not, by the allocator's choice, that of an earlier temporary -- an aliasing the log would show)
    pin = [torch.empty(a.batch, 1, a.size, a.size, device=dev) for _ in range(16)] if a.launches else None
    loss.backward()
    del pin
    h = hashlib.sha256()
    h.update(net._plans[(a.batch, a.size, a.size)].buf["logits"].detach().cpu().numpy().tobytes())
    print("logits", h.hexdigest()[:16], "loss", float(loss))
    g = hashlib.sha256()
    for k, p in sorted(net.named_parameters()):
        g.update(p.grad.detach().cpu().numpy().tobytes())
    print("grads ", g.hexdigest()[:16])
    model.eval()
    with torch.no_grad():
        ev = model(batch["input"])
    print("eval  ", hashlib.sha256(ev.cpu().numpy().tobytes()).hexdigest()[:16])
    if log is not None:
        log.close()


if __name__ == "__main__":
    main()
