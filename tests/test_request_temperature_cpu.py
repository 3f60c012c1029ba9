"""No-GPU parts of the per-request temperature ("Per-request temperature"): argument validation of
the two entry points that take 1/T per request slot, the helper that reads a temperature per prompt, and the scheduler handing each request's value
to the driver's admit."""
import ctypes

import pytest


def test_gemm_sample_batch_t_validates_without_a_gpu():
    from dflash_amd import _lib
    h = _lib.lib()
    x = _lib.RowsBatch()
    x.r0.frag, x.r0.mode, x.frag_stride = 16, 0, 4096 * 16   # a fragment source; never dereferenced: validation only

    def call(wp=16, xs=x, R=2, V=64, K=256, row0=0, nrows=16, dyn=16, ws=16, out=16, seeds=16, inv_ts=16, stream=0,
             inv_t=0.0, pos_word=3, tpr=1):
        return h.dfl_gemm_sample_batch(_lib.Weight(wp, None, _lib.W_BF16), ctypes.byref(xs) if xs is not None else None,
                                       R, V, K, row0, nrows, dyn, 2, ws, out, 16, 0, None, 0, seeds, inv_ts, inv_t, stream, pos_word, 1, tpr, None)

    assert h.dfl_gemm_sample_batch(None, None, 2, 64, 256, 0, 16, None, 2, None, None, 16, 0, None, 0, None, None, 0.0, 0, 3,
                                   1, 1, None) == -22 and b"null" in h.dfl_last_error()
    for name in ("wp", "xs", "dyn", "ws", "out", "seeds"):
        assert call(**{name: None}) == -22, name
        assert b"dfl_gemm_sample_batch: null" in h.dfl_last_error(), name
    # no per-slot array: the host inv_t (0 here) is the temperature and is range-checked
    assert call(inv_ts=None) == -22 and b"dfl_gemm_sample_batch: inv_t" in h.dfl_last_error()
    # the other checks, and -22 where the ring form does not apply
    assert call(row0=4, nrows=13) == -22 and b"rows" in h.dfl_last_error()
    assert call(stream=2) == -22 and b"stream" in h.dfl_last_error()
    assert call(pos_word=8) == -22 and call(tpr=3) == -22 and call(R=3, tpr=2) == -22
    for kw in (dict(R=5), dict(V=72), dict(K=260), dict(K=128)):
        assert call(**kw) == -22 and b"ring form" in h.dfl_last_error(), kw
    rows = _lib.RowsBatch()
    rows.r0.rows, rows.r0.mode = 16, 1                          # a row-major source has no ring form
    assert call(xs=rows) == -22 and b"ring form" in h.dfl_last_error()


def test_sample_rows_nucleus_t_validates_without_a_gpu():
    from dflash_amd import _lib
    h = _lib.lib()

    def call(logits=16, ld=64, tiles=1, V=64, row0=0, nrows=16, tpr=1, k=0, p=1.0, inv_dev=16, inv_t=0.0, stream=0, out=16):
        return h.dfl_sample_rows_nucleus(logits, ld, 1024, tiles, V, row0, nrows, None, -1, -1, 0, None, 0, tpr, None, 1,
                                         None, k, None, p, inv_dev, inv_t, stream, 0, out, 16, 0, None, None, None)

    assert call(tiles=0) == 0                                   # nothing to do: no launch; the host inv_t is not read
    assert call(logits=None) == -22 and b"dfl_sample_rows_nucleus: null" in h.dfl_last_error()
    assert call(out=None) == -22 and b"null" in h.dfl_last_error()
    assert call(p=0.0) == -22 and b"top_p" in h.dfl_last_error()
    assert call(k=-1) == -22 and call(stream=2) == -22 and call(tpr=3) == -22 and call(row0=4, nrows=13) == -22
    # without a device array the host value is the temperature, range-checked
    for it in (0.0, -1.0, 2e5, float("nan")):
        assert call(inv_dev=None, inv_t=it, tiles=0) == -22 and b"inv_t" in h.dfl_last_error(), it
    assert call(inv_dev=None, inv_t=1.0, tiles=0) == 0


def test_prompt_temperatures():
    from dflash_amd.batch import _prompt_filters, _prompt_temperatures
    assert _prompt_temperatures(0.7, 3, "torch") == ([0.7, 0.7, 0.7], False)
    assert _prompt_temperatures(0, 2, "device") == ([0.0, 0.0], False)
    assert _prompt_temperatures([0.7, 0.7], 2, "torch") == ([0.7, 0.7], False)      # equal values: today's path
    assert _prompt_temperatures((0.0, 0.7, 0.5), 3, "device") == ([0.0, 0.7, 0.5], True)
    assert _prompt_temperatures([], 0, "torch") == ([], False)
    with pytest.raises(ValueError, match="per prompt"):
        _prompt_temperatures([0.0, 0.7], 3, "device")
    with pytest.raises(ValueError, match="sampler"):
        _prompt_temperatures([0.0, 0.7], 2, "torch")
    # a filter counts where its own prompt samples
    assert _prompt_filters([5, 0], 1.0, 2, [0.0, 0.7], "device")[2] is False
    assert _prompt_filters([5, 0], 1.0, 2, [0.7, 0.0], "device")[2] is True


def test_engine_keyword_errors():
    import torch
    from dflash_amd.engine import BatchEngine
    from dflash_amd.slots import SlotLoop

    class Dec:
        max_rows, out_len = 400, 400

    eng = BatchEngine.__new__(BatchEngine)        # no GPU here: the engine's queue alone
    eng.dec, eng.temperature = Dec(), 0.7
    eng.loop = SlotLoop(eng.dec, 2, 16)
    ids = torch.zeros(1, 20, dtype=torch.int64)
    assert eng.submit(ids, 10) == 0 and eng.submit(ids, 10, temperature=0.7) == 1
    assert [r.payload.temperature for r in eng.loop.queue] == [0.7, 0.7]
    with pytest.raises(ValueError, match="request_temperature"):
        eng.submit(ids, 10, temperature=0.0)
    eng.request_temperature = True
    assert eng.submit(ids, 10, temperature=0.0, top_k=5, top_p=0.5) == 2       # a filter on a greedy request: ignored
    with pytest.raises(ValueError, match="filtering"):
        eng.submit(ids, 10, temperature=0.5, top_k=5)
    assert [r.payload.temperature for r in eng.loop.queue] == [0.7, 0.7, 0.0]


def test_slot_loop_hands_each_request_its_temperature():
    """Six requests with their own temperatures through two slots of the fake decoder of test_stream_cpu.py: the driver's
    admit sees every request's value, whichever slot it lands in."""
    from dflash_amd.slots import SlotLoop
    from test_stream_cpu import FakeDecoder

    class Plan(list):
        """An acceptance plan (what FakeDecoder reads from a payload) that carries the request's temperature."""

    class Dec(FakeDecoder):
        def __init__(self, slots):
            super().__init__(slots)
            self.admitted = []

        def admit(self, slot, request):
            self.admitted.append((request.rid, slot, request.payload.temperature))
            super().admit(slot, request)

    temps = [0.0, 0.7, 0.0, 0.5, 0.7, 1.3]
    dec = Dec(2)
    loop = SlotLoop(dec, 2, 16)
    for i, t in enumerate(temps):
        plan = Plan([0] * 16)                                   # one token per cycle
        plan.temperature = t
        loop.submit(10 + i, 2 + i, plan)
    done = loop.run()
    assert [r.rid for r in done] == list(range(6))
    assert [(rid, t) for rid, _, t in dec.admitted] == list(enumerate(temps))
    assert {s for _, s, _ in dec.admitted} == {0, 1}
