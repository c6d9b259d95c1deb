"""A recorder of the optimizer-side backend calls (adam, sgd, adam_hp, sgd_hp, grad_norm) of one engine: what TrainStep asks
the backend to launch, and over which slice of which arena.  It wraps the methods of the engine's own backend object, so it
works on the emulated backends (tests/test_optim_trace_cpu.py) and on HipBackend (tests/test_gpu_optim.py) alike, and it reads
only what every tree offers: the backend's methods and the engine's arenas."""
import json

import torch

METHODS = ("adam", "sgd", "adam_hp", "sgd_hp", "grad_norm")
STATE = ("adam_m", "adam_v", "adam_step", "adam_step_tail", "sgd_buf", "sgd_step", "grad_norm", "grad_norm_parts")


def state_present(eng):
    """which of the eight optimizer state attributes of the engine exist"""
    return [k for k in STATE if getattr(eng, k, None) is not None]


class LaunchTrace:
    """built: one entry per backend call, in call order -- the method, every positional and keyword argument (a tensor as the
    engine arena it views with its element offset and length, the rate table as its values, clip_coef=None as "none");
    ran: for every launch that ran, in order, the index in `built` of the call that made it.  patch: how the wrappers are put on the backend (monkeypatch.setattr
    where the backend outlives the test)."""

    def __init__(self, eng, patch=setattr):
        self.eng, self.built, self.ran = eng, [], []
        for name in METHODS:
            patch(eng.be, name, self._wrap(name, getattr(eng.be, name)))

    def _wrap(self, name, method):
        def call(*args, **kwargs):
            kw = {k: ("none" if k == "clip_coef" and v is None else self._arg(v)) for k, v in kwargs.items()}
            index = len(self.built)
            self.built.append({"call": name, "args": [self._arg(a) for a in args], "kwargs": kw})
            run = method(*args, **kwargs)

            def noted(stream):
                self.ran.append(index)
                return run(stream)
            return noted
        return call

    def _arg(self, a):
        if not isinstance(a, torch.Tensor):
            return a
        arenas = {"P": self.eng.P.data, "G": self.eng.G}
        arenas.update({k: getattr(self.eng, k) for k in STATE if getattr(self.eng, k, None) is not None})
        for k, t in arenas.items():
            if t.untyped_storage().data_ptr() == a.untyped_storage().data_ptr():
                assert a.is_contiguous() and a.dtype == t.dtype, k
                return {"arena": k, "offset": a.storage_offset() - t.storage_offset(), "len": a.numel()}
        assert a.dtype == torch.float32 and a.dim() == 1, "a tensor that views no arena is the rate table"
        return {"table": a.tolist()}

    def take(self):
        """the trace so far as plain JSON values; the recorder starts again"""
        out = json.loads(json.dumps({"built": self.built, "ran": self.ran}))
        self.built, self.ran = [], []
        return out
