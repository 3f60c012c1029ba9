"""Every launch of the verify's logits chain, with its arguments: the configurations of
tests/test_hip_logits_stage.py — all six features in a DecodeSession and in a BatchedDecoder, each feature alone and
none, at T = 0.7 and T = 0 — under that file's recorder.  Per call of a chain entry (head launch, row processors, draw,
logprobs, accept, count, advance, and dfl_sample_rows): the entry's name and its arguments, every pointer replaced by
the ordinal of its first appearance in the configuration's run, floats by their repr.  Every tensor whose address is
taken stays alive until its configuration is printed, so that the allocator never hands a freed buffer's address to
another one and an ordinal names one buffer.  Two revisions of the package that print the same text enqueue the same
launches on the same buffers.

    timeout -k 10 600 python scripts/trace_logits_stage.py > trace.txt
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_hip_logits_stage as TS  # noqa: E402
from dflash_amd import _lib  # noqa: E402

TRACED = TS.CHAIN + ("dfl_sample_rows",)


class Ordinals:
    def __init__(self):
        self.seen = {}

    def ptr(self, v):
        if not v:
            return "null"
        return f"p{self.seen.setdefault(int(v), len(self.seen))}"

    def value(self, v, ctype):
        if ctype is C.c_void_p:
            return self.ptr(v)
        if isinstance(ctype, type) and issubclass(ctype, C.Structure):
            return "{" + " ".join(f"{n}={self.value(getattr(v, n), t)}" for n, t in ctype._fields_) + "}"
        if isinstance(ctype, type) and issubclass(ctype, C._Pointer):   # a descriptor handed over by reference
            if v is None:
                return "null"
            return self.value(v if isinstance(v, C.Structure) else v._obj, ctype._type_)
        return repr(float(v)) if ctype is C.c_float else repr(int(v))

    def call(self, name, args):
        types = _lib.SIGNATURES[name][1]
        return f"{name}(" + ", ".join(self.value(a, t) for a, t in zip(args, types)) + ")"


def dump(title, parts):
    print(f"== {title}")
    o = Ordinals()
    for label, calls in parts:
        print(f"-- {label}")
        for name, args in calls:
            if name in TRACED:
                print("   " + o.call(name, args))


def main():
    real = _lib.lib()
    rec = TS.Recorder(real)
    _lib._lib = rec
    torch.manual_seed(0)
    keep, data_ptr = [], torch.Tensor.data_ptr

    def kept_data_ptr(t):
        keep.append(t)
        return data_ptr(t)

    torch.Tensor.data_ptr = kept_data_ptr
    try:
        cases = [(TS.FEATURES, TS.T)] + [((f,), t) for f in TS.FEATURES for t in (TS.T, 0.0)] + [((), TS.T), ((), 0.0)]
        for on, t in cases:
            name = "+".join(on) or "none"
            first, cycle, _ = TS.run_session(rec, on, t)
            dump(f"session {name} T={t}", [("prefill", first), ("cycle", cycle)])
            admits, cycle, _ = TS.run_decoder(rec, on, t, request_temperature=on == TS.FEATURES)
            dump(f"decoder {name} T={t}", [("admit 0", admits[0]), ("admit 1", admits[1]), ("cycle", cycle)])
            keep.clear()
    finally:
        _lib._lib, torch.Tensor.data_ptr = real, data_ptr


if __name__ == "__main__":
    main()
