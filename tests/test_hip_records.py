"""The integer records that steer a replayed decode cycle, and the small row movers beside them, against the plain
model of records_ref.py.  Everything is compared exactly.  Every buffer a kernel may write is wider than the kernel is
told (extra slots, row strides above the logical width), pre-filled with distinct sentinels, and compared WHOLE, so a
write one word past a record, one id past output_len or into a neighbouring slot fails."""
import pytest
import torch

import helpers as H
import records_ref as RR

pytestmark = pytest.mark.gpu

I32, I64, BF16, F32 = torch.int32, torch.int64, torch.bfloat16, torch.float32
MASK = 151669
EINVAL = -22


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops as o
    return o


def dev():
    return torch.device("cuda", 0)


def stream():
    return torch.cuda.current_stream().cuda_stream


def sent(shape, base, dtype=I64):
    """Distinct sentinel values base, base + 1, ... (none is a token id, a mask id or a plausible length)."""
    n = 1
    for s in shape:
        n *= s
    return (torch.arange(n, dtype=I64) + base).to(dtype).reshape(shape)


def same(name, got: torch.Tensor, want) -> None:
    got = got.cpu().tolist()
    if got != want:
        flat_g = torch.tensor(got).flatten().tolist()
        flat_w = torch.tensor(want).flatten().tolist()
        bad = [(i, g, w) for i, (g, w) in enumerate(zip(flat_g, flat_w)) if g != w][:8]
        raise AssertionError(f"{name}: kernel != reference at flat (index, kernel, reference): {bad}")


def pair_rows(bs, acc, blk_w, post_w, base):
    """One request's block / posterior rows at their full strides, first mismatch exactly at `acc`; every later
    position matches again, past bs too, so that counting all matches or ignoring bs shows."""
    block = [base + i for i in range(blk_w)]
    post = [block[i + 1] if i + 1 < blk_w else base + 700 + i for i in range(post_w)]
    if bs >= 1 and acc < bs - 1:
        post[acc] = base + 500
    return block, post


class Batch:
    """Host lists (the reference's state) and device tensors of one ragged batch, R requests in R + 1 slots."""

    def __init__(self, R, blk_stride, post_stride, out_len, out_stride, tpr=1, separate=False, alias_tiles=False):
        self.R, self.tpr, self.out_len = R, tpr, out_len
        n = R + 1
        self.h = {"block": sent((n, blk_stride), 7_000_000).tolist(), "post": sent((n, post_stride), 7_100_000).tolist(),
                  "out": sent((n, out_stride), 7_200_000).tolist(), "dyn_d": sent((n, 8), 5000, I32).tolist(),
                  "dyn_t": sent((n, 8), 5200, I32).tolist(), "result": sent((n, 4), 5400, I32).tolist()}
        if separate:
            self.h["nb"] = sent((n, blk_stride), 7_300_000).tolist()
        if tpr == 2 or not alias_tiles:
            self.h["dyn_dt"] = sent((n * tpr, 8), 5600, I32).tolist()
            self.h["dyn_tt"] = sent((n * tpr, 8), 5800, I32).tolist()
        self.alias = alias_tiles and tpr == 1
        self.g = {}

    def upload(self, *names):
        for k in names or self.h:
            dt = I32 if k.startswith("dyn") or k == "result" else I64
            self.g[k] = torch.tensor(self.h[k], dtype=dt, device=dev())

    def tiles(self, side):
        """(host, device) per-tile records: the per-request ones themselves when aliased."""
        if self.alias:
            return (self.h["dyn_d"], self.g["dyn_d"]) if side == "d" else (self.h["dyn_t"], self.g["dyn_t"])
        return (self.h["dyn_dt"], self.g["dyn_dt"]) if side == "d" else (self.h["dyn_tt"], self.g["dyn_tt"])

    def launch(self, ops, stops=(), rearm="inplace", tiled=False):
        """One accept launch on the device and the same step of the reference; rearm: 'inplace', 'separate' or None."""
        g, h, R = self.g, self.h, self.R
        st = torch.tensor(list(stops), dtype=I64, device=dev()) if stops else None
        nb_g = {"inplace": g["block"], "separate": g.get("nb"), None: None}[rearm]
        nb_h = {"inplace": h["block"], "separate": h.get("nb"), None: None}[rearm]
        hd = ht = None
        if tiled:
            (hd, gd), (ht, gt) = self.tiles("d"), self.tiles("t")
        if tiled and self.tpr == 1:      # the wrapper hands over no tile records for one tile per request: call the library
            L = ops.lib()
            rc = L.dfl_accept_commit_batch(
                g["block"].data_ptr(), g["block"].stride(0), g["post"].data_ptr(), g["post"].stride(0), R,
                g["out"].data_ptr(), g["out"].stride(0), self.out_len, g["dyn_d"].data_ptr(), g["dyn_t"].data_ptr(),
                st.data_ptr() if stops else None, len(stops), g["result"].data_ptr(),
                nb_g.data_ptr() if nb_g is not None else None, MASK, 1, gd.data_ptr(), gt.data_ptr(), stream())
            assert rc == 0, L.dfl_last_error()
        else:
            ops.accept_commit_batch(g["block"], g["post"], R, g["out"], g["dyn_d"], g["dyn_t"], st, g["result"],
                                    rearm_mask_id=None if rearm is None else MASK, tiles_per_req=self.tpr,
                                    dyn_d_tiles=gd if tiled else None, dyn_t_tiles=gt if tiled else None,
                                    next_block=nb_g if rearm == "separate" else None, output_len=self.out_len)
        return RR.batch_cycle(R, h["block"], h["post"], h["out"], self.out_len, h["dyn_d"], h["dyn_t"], stops, h["result"],
                              nb_h, MASK, self.tpr, hd, ht)

    def check(self, what=""):
        torch.cuda.synchronize()
        for k in self.h:
            same(f"{what} {k}", self.g[k], self.h[k])

    def arm(self, r, bs, acc, start, base, stop=0, cycle=3):
        h = self.h
        h["block"][r], h["post"][r] = pair_rows(bs, acc, len(h["block"][r]), len(h["post"][r]), base)
        h["dyn_d"][r][RR.BS], h["dyn_d"][r][RR.START] = bs, start
        h["dyn_d"][r][RR.STOP], h["dyn_d"][r][RR.CYCLE] = stop, cycle


# ---- a. dfl_accept_commit_batch, one cycle ------------------------------------------------------------------------
BS_SET = [0, 1, 2, 9, 16]


@pytest.mark.parametrize("blk_stride,post_stride,rearm", [(16, 16, "inplace"), (24, 40, "separate"), (24, 16, None),
                                                          (16, 24, "separate")])
@pytest.mark.parametrize("R", [1, 3, 4, 7])
def test_accept_commit_batch_one_cycle(ops, R, blk_stride, post_stride, rearm):
    """Every bs of {0, 1, 2, 9, 16} in every slot position, acc forced to each of {0, 1, bs - 2, bs - 1}, an idle slot
    in every launch of R >= 3; out_stride = output_len + 5; block re-armed in place, elsewhere, or not at all."""
    out_len = 64
    for rot in range(5):
        for kind in range(4):
            b = Batch(R, blk_stride, post_stride, out_len, out_len + 5, separate=rearm == "separate")
            bss = [BS_SET[(r + rot) % 5] for r in range(R)]
            if R >= 3 and 0 not in bss:
                bss[(rot + kind) % R] = 0
            want = []
            for r, bs in enumerate(bss):
                acc = max(0, min(bs - 1, [0, 1, bs - 2, bs - 1][(kind + r) % 4]))
                want.append(acc if bs else None)
                b.arm(r, bs, acc, 5 + 3 * r, 1000 * (r + 1), cycle=3 + r)
            b.upload()
            assert b.launch(ops, rearm=rearm) == want        # the reference sees the mismatch where it was planted
            b.check(f"R={R} bs={bss} acc={want}")


# ---- b. dfl_accept_commit_batch, tiled -----------------------------------------------------------------------------
@pytest.mark.parametrize("blk_stride,post_stride,rearm", [(32, 32, "inplace"), (40, 48, "separate")])
def test_accept_commit_batch_t_two_tiles(ops, blk_stride, post_stride, rearm):
    """Blocks of 17..32 rows, a wide slot running a short tail block (bs 16, 5: tile 1's shares are 0) and an idle slot,
    with acc + 1 on and around the tile boundary; both per-tile records whole; the re-armed block is 32 wide."""
    cases = [(bs, t - 1) for bs in (17, 24, 31, 32, 16, 5) for t in (1, 15, 16, 17, 31, 32) if t <= bs]
    cases += [(0, 0)] * (-len(cases) % 2)
    for k in range(0, len(cases), 2):
        b = Batch(3, blk_stride, post_stride, 200, 205, tpr=2, separate=rearm == "separate")
        trio = [cases[k], (0, 0), cases[k + 1]]                 # the idle slot sits between two busy ones
        for r, (bs, acc) in enumerate(trio):
            b.arm(r, bs, acc, 40 + 7 * r, 1000 * (r + 1))
        b.upload()
        assert b.launch(ops, rearm=rearm, tiled=True) == [c[1] if c[0] else None for c in trio]
        for r, (bs, acc) in enumerate(trio):
            if bs:                                              # said outright, besides the model: the tiles' shares
                dd, dt = b.h["dyn_dt"], b.h["dyn_tt"]
                assert [dd[2 * r + j][RR.TAU] for j in (0, 1)] == [min(acc + 1, 16), max(0, acc + 1 - 16)]
                assert [dt[2 * r + j][RR.BS] for j in (0, 1)] == [min(bs, 16), max(0, bs - 16)]
                assert dd[2 * r + 1][RR.S] == 40 + 7 * r + 16
        b.check(f"tiles {trio}")


def test_accept_commit_batch_t_one_tile_equals_batch(ops):
    """tiles_per_req = 1 with the per-tile pointers being the per-request records, as the batched decoder holds them:
    exactly what dfl_accept_commit_batch leaves without tile records."""
    for kind in range(4):
        pairs = []
        for tiled in (False, True):
            b = Batch(4, 16, 16, 64, 69, alias_tiles=True)
            for r in range(4):
                bs = BS_SET[(r + kind) % 5]
                b.arm(r, bs, max(0, min(bs - 1, [0, 1, bs - 2, bs - 1][(kind + r) % 4])), 9 + r, 1000 * (r + 1))
            b.upload()
            b.launch(ops, stops=(1001,), tiled=tiled)
            b.check(f"tiled={tiled}")
            pairs.append({k: v.cpu() for k, v in b.g.items()})
        assert pairs[0].keys() == pairs[1].keys()
        for k in pairs[0]:
            assert torch.equal(pairs[0][k], pairs[1][k]), k


# ---- c. clipping and stop ids -------------------------------------------------------------------------------------
def test_clipping_batch_and_single(ops):
    """start + acc + 1 reaches output_len by 0, 1 and acc + 1 tokens: ids past output_len untouched, new start and tau
    still count the clipped tokens, a clipped stop id still stops."""
    bs, acc, out_len = 9, 4, 50
    overs = (0, 1, acc + 1)
    b = Batch(3, 16, 16, out_len, out_len + 5)
    for r, over in enumerate(overs):
        b.arm(r, bs, acc, out_len + over - acc - 1, 1000 * (r + 1))
    b.upload()
    bonus2 = b.h["post"][2][acc]
    assert b.launch(ops, stops=(bonus2,)) == [acc] * 3
    for r, over in enumerate(overs):
        assert b.h["dyn_d"][r][RR.START] == out_len + over and b.h["dyn_d"][r][RR.TAU] == acc + 1
        assert b.h["out"][r][out_len:] == sent((4, out_len + 5), 7_200_000)[r, out_len:].tolist()
    assert [b.h["dyn_d"][r][RR.STOP] for r in range(3)] == [0, 0, 1]       # slot 2's bonus token is clipped, and stops
    b.check("clipping, batch form")
    for over in overs:
        for form in ("plain", "rearm", "rearm_t"):
            s = Single(bs, acc, out_len + over - acc - 1, out_len)
            s.run(ops, form, stops=(s.post[acc],))
            assert s.dyn[8 + RR.START] == out_len + over and s.dyn[8 + RR.STOP] == 1
            s.check(f"clipping, single {form} over={over}")


STOP_CASES = [  # (which token of slot 1 is the stop id, n_stop, hit?)   bs = 6, acc = 2: block[0..2] + post[2] written
    ("block", 0, 1, 1), ("block", 1, 1, 1), ("block", 2, 3, 1), ("post", 2, 1, 1), ("post", 2, 3, 1),
    ("block", 3, 1, 0), ("block", 4, 3, 0), ("post", 3, 1, 0), ("post", 5, 3, 0), ("block", 0, 0, 0)]


@pytest.mark.parametrize("which,idx,n_stop,hit", STOP_CASES)
def test_stop_ids_batch_and_single(ops, which, idx, n_stop, hit):
    """Hit by block[0], an accepted draft token, the bonus token; not by a rejected draft token nor by post[i > acc];
    n_stop 0 (NULL), 1, 3; sticky over a following cycle without a hit; per slot; mirrored into dyn_t and result."""
    bs, acc = 6, 2
    b = Batch(3, 16, 16, 64, 69)
    for r in range(3):
        b.arm(r, bs, acc, 10 + r, 1000 * (r + 1), stop=0)
    tok = b.h[which][1][idx]
    stops = ([], [tok], None, [31, tok, 32])[n_stop]
    b.upload()
    b.launch(ops, stops=stops)
    b.check("stop, cycle 1")
    flags = [0, hit, 0]
    for cyc in (1, 2):
        assert [d[RR.STOP] for d in b.h["dyn_d"][:3]] == flags and [d[RR.STOP] for d in b.h["dyn_t"][:3]] == flags
        assert [x[2] for x in b.h["result"][:3]] == flags
        if cyc == 1:                                   # a second cycle with fresh tokens, none a stop id
            for r in range(3):
                b.h["block"][r], b.h["post"][r] = pair_rows(bs, 1, 16, 16, 1000 * (r + 1) + 100)
            b.upload("block", "post")
            b.launch(ops, stops=stops)
            b.check("stop, cycle 2")
    for form in ("plain", "rearm", "rearm_t"):
        s = Single(bs, acc, 10, 64, base=2000)
        s.run(ops, form, stops=stops)
        assert s.dyn[8 + RR.STOP] == hit and s.res[4 + 2] == hit
        s.check(f"stop, single {form}")
        s.block[:16], s.post[:16] = pair_rows(bs, 1, 16, 16, 2100)
        s.upload()
        s.run(ops, form, stops=stops)
        assert s.dyn[8 + RR.STOP] == hit and s.dyn[8 + RR.CYCLE] == 5
        s.check(f"stop, single {form}, cycle 2")


# ---- e. single form (also used by c) ------------------------------------------------------------------------------
class Single:
    """One request through dfl_accept_commit (plain / re-arm / re-arm with dyn_t): the records sit inside 24-word sentinel buffers
    (dyn at word 8, result at word 4), block / posterior / ids in buffers wider than bs and output_len."""

    def __init__(self, bs, acc, start, out_len, base=1000, width=72):
        self.bs, self.out_len = bs, out_len
        self.block, self.post = pair_rows(bs, acc, width, width, base)
        self.out = sent((out_len + 7,), 7_200_000).tolist()
        self.dyn, self.dyn_t, self.res = (sent((24,), b, I32).tolist() for b in (5000, 5200, 5400))
        self.dyn[8:16] = [5008, 5009, 5010, 5011, start, 0, 3, 5015]
        self.upload()

    def upload(self):
        self.g = {k: torch.tensor(getattr(self, k), dtype=I32 if k in ("dyn", "dyn_t", "res") else I64, device=dev())
                  for k in ("block", "post", "out", "dyn", "dyn_t", "res")}

    def run(self, ops, form, stops=(), rearm_n=64):
        g = self.g
        st = torch.tensor(list(stops), dtype=I64, device=dev()) if stops else None
        dyn, dyn_t, res = self.dyn[8:16], self.dyn_t[8:16], self.res[4:8]
        ops.accept_commit(g["block"], g["post"], self.bs, g["out"][:self.out_len], g["dyn"][8:16], st, g["res"][4:8],
                          rearm=None if form == "plain" else (g["block"], rearm_n, MASK),
                          dyn_t=g["dyn_t"][8:16] if form == "rearm_t" else None)
        acc = RR.single_cycle(self.block, self.post, self.bs, self.out, self.out_len, dyn, stops or (), res,
                              None if form == "plain" else self.block, rearm_n, MASK, dyn_t if form == "rearm_t" else None)
        self.dyn[8:16], self.dyn_t[8:16], self.res[4:8] = dyn, dyn_t, res
        return acc

    def check(self, what):
        torch.cuda.synchronize()
        for k in self.g:
            same(f"{what} {k}", self.g[k], getattr(self, k))


@pytest.mark.parametrize("bs", [17, 32, 33, 63])
def test_accept_commit_single_beyond_goldens(ops, bs):
    """bs above the goldens' 16, acc 0, 31, 32 and bs - 1 (bs = 63, acc = 62: lane 63 writes the bonus token)."""
    for acc in sorted({a for a in (0, 31, 32, bs - 1) if a <= bs - 1}):
        for form in ("plain", "rearm", "rearm_t"):
            s = Single(bs, acc, 21, 120)
            assert s.run(ops, form) == acc
            assert s.out[21 + acc + 1] == s.post[acc] if form == "plain" else s.block[0] == s.out[21 + acc + 1]
            s.check(f"single {form} bs={bs} acc={acc}")


# ---- d. forty cycles ----------------------------------------------------------------------------------------------
def _tape(r, pos):
    return 100 + (pos * 37 + r * 1009) % 90001        # consecutive positions differ; never MASK, never a sentinel


@pytest.mark.parametrize("tpr", [1, 2])
def test_forty_cycles_against_the_model(ops, tpr):
    """R = 4 over 40 cycles of a seeded acceptance plan, the block of each cycle built on the host from the re-armed
    block the kernel left.  Slot 1 is parked at cycle 10 and slot 2's block size lowered at cycle 20, as the batched
    decoder writes them; at one tile per request slot 1 is re-admitted by dfl_admit_slot at cycle 25 over its dirty
    state.  All records, ids and results equal the model's after every cycle."""
    R, BW = 4, 16 * tpr
    out_len = 40 * BW + 64
    blk_stride, post_stride = (16, 16) if tpr == 1 else (40, 32)
    b = Batch(R, blk_stride, post_stride, out_len, out_len + 5, tpr=tpr, alias_tiles=True)
    h = b.h
    bss = [BW, BW - 3, BW, 17 * tpr - 16]                     # 16 13 16 1  |  32 29 32 18
    seeds = sent((R + 1,), 900).tolist()
    fc_in = 64
    taps = torch.full((R + 1, 16, fc_in), float("nan"), dtype=BF16).to(dev())
    for r in range(R):                                        # the state an admission leaves
        prompt = [_tape(r, p) for p in range(5 + 3 * r)]
        RR.admit(prompt, _tape(r, len(prompt)), h["out"][r], out_len, h["block"][r], h["post"][r], BW,
                 h["result"][r], min(16, len(prompt)), h["dyn_d"][r], h["dyn_t"][r], bss[r], MASK)
        if tpr == 2:
            P, n_tail = len(prompt), min(16, len(prompt))
            for j in range(2):
                h["dyn_dt"][2 * r + j] = [P - n_tail + 16 * j, n_tail if j == 0 else 0, 0, P - n_tail + 16 * j, P, 0, 0, 0]
                h["dyn_tt"][2 * r + j] = [P, 0, RR.clamp(bss[r] - 16 * j, 0, 16), P, P, 0, 0, 0]
    b.upload()
    plans = [H.make_plan(40, BW, 50 + r) for r in range(R)]
    stops = (_tape(3, 40), 11, 12)
    for c in range(40):
        if c == 10:                                           # BatchedDecoder.park(1)
            h["dyn_d"][1][RR.TAU] = h["dyn_d"][1][RR.BS] = h["dyn_t"][1][RR.BS] = 0
            if tpr == 2:
                for t in (2, 3):
                    h["dyn_dt"][t][RR.TAU] = h["dyn_dt"][t][RR.BS] = h["dyn_tt"][t][RR.BS] = 0
        if c == 20:                                           # BatchedDecoder.set_block_size(2, ...)
            nbs = 7 if tpr == 1 else 12
            h["dyn_d"][2][RR.BS] = h["dyn_t"][2][RR.BS] = nbs
            if tpr == 2:
                h["dyn_tt"][4][RR.BS], h["dyn_tt"][5][RR.BS] = min(nbs, 16), max(0, nbs - 16)
        if c == 25 and tpr == 1:                              # slot 1 again, over what the parked request left
            prompt = [_tape(1, 3000 + p) for p in range(19)]
            pr = torch.tensor(prompt, dtype=I64, device=dev())
            first = torch.tensor([_tape(1, 3019)], dtype=I64, device=dev())
            tail = torch.ones(16, fc_in, dtype=BF16, device=dev())
            sd = torch.tensor(seeds, dtype=I64, device=dev())
            g = b.g
            rc = ops.lib().dfl_admit_slot(1, R, pr.data_ptr(), 19, first.data_ptr(), g["out"].data_ptr(), out_len + 5,
                                          out_len, g["block"].data_ptr(), g["post"].data_ptr(), 16, g["result"].data_ptr(),
                                          tail.data_ptr(), fc_in, 16, taps.data_ptr(), fc_in, g["dyn_d"].data_ptr(),
                                          g["dyn_t"].data_ptr(), 9, sd.data_ptr(), 777, MASK, stream())
            assert rc == 0, ops.lib().dfl_last_error()
            RR.admit(prompt, _tape(1, 3019), h["out"][1], out_len, h["block"][1], h["post"][1], 16, h["result"][1], 16,
                     h["dyn_d"][1], h["dyn_t"][1], 9, MASK, seeds, 1, 777)
            b.check("after admit")
            same("seeds", sd, seeds)
            assert torch.equal(taps[1].view(torch.int16).cpu(), torch.ones(16, fc_in, dtype=BF16).view(torch.int16))
        if c in (10, 20):
            b.upload(*[k for k in h if k.startswith("dyn")])
        # the host's part of a cycle: draft tokens into the re-armed block, the target's tokens into post
        for r in range(R):
            bs, start = h["dyn_d"][r][RR.BS], h["dyn_d"][r][RR.START]
            if bs == 0:
                continue
            shift = 3000 - 19 if (r == 1 and c >= 25) else 0      # slot 1's second request: position p holds tape 2981 + p
            assert h["block"][r][:BW] == [h["out"][r][start] if start < out_len else h["block"][r][0]] + [MASK] * (BW - 1)
            k = min(plans[r][c], bs - 1)
            for i in range(bs):
                tok = _tape(r, start + 1 + i + shift)
                h["post"][r][i] = tok
                if i + 1 < bs:
                    h["block"][r][i + 1] = tok + 1 if i == k else tok
        b.upload("block", "post")
        accs = b.launch(ops, stops=stops, tiled=tpr == 2)
        for r in range(R):
            if accs[r] is not None:
                assert accs[r] == min(plans[r][c], h["dyn_t"][r][RR.BS] - 1)
        b.check(f"cycle {c}")
    assert [d[RR.CYCLE] for d in h["dyn_d"][:R]] == ([40, 15, 40, 40] if tpr == 1 else [40, 10, 40, 40])
    assert h["dyn_d"][3][RR.STOP] == 1 and h["dyn_d"][0][RR.STOP] == 0


# ---- f. dfl_admit_slot ----------------------------------------------------------------------------------------------
class Admit:
    """Three slots in four-slot buffers, all dirty: ids, block, post, result, records, seeds hold sentinels and the
    context tiles NaN."""

    def __init__(self, P, n_tail, fc_in, out_len, blk_w, seed_given=True):
        self.P, self.n_tail, self.fc_in, self.out_len, self.blk_w = P, n_tail, fc_in, out_len, blk_w
        n = 4
        self.h = {"out": sent((n, out_len + 3), 7_200_000).tolist(), "block": sent((n, blk_w), 7_000_000).tolist(),
                  "post": sent((n, blk_w), 7_100_000).tolist(), "result": sent((n, 4), 5400, I32).tolist(),
                  "dyn_d": sent((n, 8), 5000, I32).tolist(), "dyn_t": sent((n, 8), 5200, I32).tolist(),
                  "seeds": sent((n,), 900).tolist()}
        self.g = {k: torch.tensor(v, dtype=I32 if k in ("result", "dyn_d", "dyn_t") else I64, device=dev())
                  for k, v in self.h.items()}
        self.taps = torch.full((n, 16, fc_in), float("nan"), dtype=BF16).to(dev())
        self.prompt = [200 + 3 * i for i in range(P)]
        self.pr = torch.tensor(self.prompt or [0], dtype=I64, device=dev())
        self.first = torch.tensor([4242], dtype=I64, device=dev())
        self.ld = fc_in + 64                                   # the tail is a column view of a wider tensor
        g = H.gen(P + fc_in + n_tail)
        self.wide = torch.randint(-3, 4, (16, self.ld), generator=g).to(BF16).to(dev())
        self.seed_given = seed_given

    def call(self, ops, r, bs, n_slots=3, P=None, n_tail=None, out_len=None, blk_w=None, fc_in=None, ld=None, tail_off=32):
        g = self.g
        tail_ptr = self.wide.data_ptr() + 2 * tail_off
        return ops.lib().dfl_admit_slot(
            r, n_slots, self.pr.data_ptr(), self.P if P is None else P, self.first.data_ptr(), g["out"].data_ptr(),
            self.out_len + 3, self.out_len if out_len is None else out_len, g["block"].data_ptr(), g["post"].data_ptr(),
            self.blk_w if blk_w is None else blk_w, g["result"].data_ptr(), tail_ptr, self.ld if ld is None else ld,
            self.n_tail if n_tail is None else n_tail, self.taps.data_ptr(), self.fc_in if fc_in is None else fc_in,
            g["dyn_d"].data_ptr(), g["dyn_t"].data_ptr(), bs, g["seeds"].data_ptr() if self.seed_given else None, 31337,
            MASK, stream())

    def want_taps(self, r, rows):
        t = torch.full((4, 16, self.fc_in), float("nan"), dtype=BF16)
        t[r] = 0
        for i, src in enumerate(rows):
            if src is not None:
                t[r, i] = self.wide[src, 32:32 + self.fc_in].cpu()
        return t.view(torch.int16)

    def check(self, what, want_taps):
        torch.cuda.synchronize()
        for k in self.h:
            same(f"{what} {k}", self.g[k], self.h[k])
        assert torch.equal(self.taps.cpu().view(torch.int16), want_taps), f"{what}: context tiles differ"


ADMIT_CASES = [  # P, n_tail, fc_in, out_len - P (0: 40000 ids), blk_w, bs, r, seed given
    (1, 0, 8, 1, 1, 0, 0, True), (1, 1, 8, 40, 1, 1, 2, False), (5, 0, 2560, 40, 16, 16, 0, True),
    (5, 1, 8, 1, 16, 0, 2, False), (16, 15, 8, 40, 32, 32, 0, True), (16, 16, 2560, 0, 64, 1, 2, True),
    (17, 16, 20480, 40, 64, 64, 0, False), (17, 15, 8, 1, 32, 1, 2, True), (300, 16, 2560, 1, 16, 1, 0, False),
    (300, 0, 20480, 0, 32, 0, 2, True), (300, 1, 8, 40, 64, 64, 2, True), (5, 1, 20480, 40, 1, 0, 0, True)]


@pytest.mark.parametrize("P,n_tail,fc_in,room,blk_w,bs,r,seed_given", ADMIT_CASES)
def test_admit_slot_direct(ops, P, n_tail, fc_in, room, blk_w, bs, r, seed_given):
    """dfl_admit_slot without a model, from a dirty slot: ids, block, post / result, both records whole, the seed, and
    the 16 x fc_in context tile bit for bit (tail rows copied, the rest zero, not NaN); the other slots untouched."""
    out_len = P + room if room else 40000
    a = Admit(P, n_tail, fc_in, out_len, blk_w, seed_given)
    assert a.call(ops, r, bs) == 0, ops.lib().dfl_last_error()
    h = a.h
    rows = RR.admit(a.prompt, 4242, h["out"][r], out_len, h["block"][r], h["post"][r], blk_w, h["result"][r], n_tail,
                    h["dyn_d"][r], h["dyn_t"][r], bs, MASK, h["seeds"] if seed_given else None, r, 31337)
    assert h["out"][r][P] == 4242 and (room == 1 or h["out"][r][P + 1] == MASK)
    a.check(f"admit P={P} n_tail={n_tail} fc_in={fc_in}", a.want_taps(r, rows))


def test_admit_slot_rejections(ops):
    """Each bad argument returns DFL_EINVAL before any launch: nothing on the device changes."""
    a = Admit(20, 16, 64, 60, 16)
    nan_taps = torch.full((4, 16, 64), float("nan"), dtype=BF16).view(torch.int16)
    bad = [dict(r=3), dict(P=0, n_tail=0), dict(out_len=20), dict(P=9, n_tail=10), dict(n_tail=17), dict(bs=17),
           dict(fc_in=12), dict(ld=64 + 68), dict(tail_off=33), dict(r=-1), dict(bs=-1), dict(blk_w=65)]
    for kw in bad:
        kw = {"r": 1, "bs": 16, **kw}
        assert a.call(ops, **kw) == EINVAL, kw
        a.check(f"rejected {kw}", nan_taps)
    assert a.call(ops, 1, 16) == 0                           # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert a.g["dyn_t"][1].tolist() == [20, 0, 16, 20, 20, 0, 0, 0]


# ---- g. dfl_set_dyn / dfl_set_dyn2 ----------------------------------------------------------------------------------
def test_set_dyn_into_dirty_records(ops):
    for (s, tau, bs, pos0) in [(40, 3, 16, 40), (0, 0, 0, 0), (7, 0, 63, 12), (100, 16, 1, 90), (5, 9, 0, 77)]:
        want = sent((24,), 5000, I32).tolist()
        buf = torch.tensor(want, dtype=I32, device=dev())
        ops.set_dyn(buf[8:16], s, tau, bs, pos0)
        rec = want[8:16]
        RR.set_dyn(rec, s, tau, bs, pos0)
        want[8:16] = rec
        assert want[8 + RR.START] == pos0 + tau and want[13:16] == [0, 0, 0]
        same(f"set_dyn {(s, tau, bs, pos0)}", buf, want)
    buf = sent((24,), 5000, I32).to(dev())
    for args in [(1, 1, 64, 1), (-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, 1, -1)]:
        with pytest.raises(RuntimeError):
            ops.set_dyn(buf[8:16], *args)
    same("set_dyn rejected", buf, sent((24,), 5000, I32).tolist())


def test_set_dyn2_clamps_both_tiles(ops):
    for tau in (0, 1, 16, 17, 32):
        for bs in (0, 1, 16, 17, 32):
            want = sent((24,), 5000, I32).tolist()
            buf = torch.tensor(want, dtype=I32, device=dev())
            ops.set_dyn2(buf[4:], 11, tau, bs, 30)
            recs = want[4:20]
            RR.set_dyn2(recs, 11, tau, bs, 30)
            want[4:20] = recs
            assert want[4 + RR.START] == want[12 + RR.START] == 30 + tau                  # unclamped in both
            assert want[4 + RR.TAU] + want[12 + RR.TAU] == tau and want[4 + RR.BS] + want[12 + RR.BS] == bs
            same(f"set_dyn2 tau={tau} bs={bs}", buf, want)
    buf = sent((24,), 5000, I32).to(dev())
    for args in [(1, 33, 1, 1), (1, 1, 33, 1), (-1, 1, 1, 1)]:
        with pytest.raises(RuntimeError):
            ops.set_dyn2(buf[4:], *args)
    same("set_dyn2 rejected", buf, sent((24,), 5000, I32).tolist())


# ---- h. dfl_embed_rows_batch, dfl_embed_rows ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables():
    """Embedding tables of small integers (|v| <= 3): every sum of squares is exact in fp32 in any order."""
    return {Hd: torch.randint(-3, 4, (1000, Hd), generator=H.gen(Hd)).to(BF16) for Hd in (8, 2560, 4096)}


def _i16(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("ids_stride", [16, 40])
@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("Hd", [8, 2560, 4096])
def test_embed_rows_batch(ops, tables, Hd, R, ids_stride):
    """Rows below the request's count bit-equal to embed[ids] and ss == the exact sum of squares; rows at or past it
    keep their NaN and get ss exactly 0; nothing outside the strides' logical part is touched."""
    emb = tables[Hd]
    counts = [16, 0, 7, 1]
    ids = torch.randint(0, 1000, (R + 1, ids_stride), generator=H.gen(R + ids_stride))
    ids[0, 0], ids[0, 1], ids[R - 1, 6] = 0, 999, 999
    h_stride, ss_stride = 16 * Hd + 64, 24
    dyn = sent((R + 1, 8), 5000, I32)
    dyn[:R, RR.BS] = torch.tensor(counts[:R], dtype=I32)
    hbuf = torch.full(((R + 1) * h_stride,), float("nan"), dtype=BF16).to(dev())
    ssbuf = sent((R + 1, ss_stride), 100).to(F32).to(dev())
    hv = hbuf.as_strided((R, 16, Hd), (h_stride, Hd, 1))
    ops.embed_rows_batch(emb.to(dev()), ids.to(dev()), R, hv, Hd, ssbuf[:R], dyn.to(dev()), RR.BS)
    want_h = torch.full(((R + 1), h_stride), float("nan"), dtype=BF16)
    want_ss = sent((R + 1, ss_stride), 100).to(F32)
    for r in range(R):
        n = counts[r]
        rows = emb[ids[r, :n]]
        want_h[r, :n * Hd] = rows.reshape(-1)
        want_ss[r, :16] = 0
        want_ss[r, :n] = rows.double().pow(2).sum(-1).float()
    torch.cuda.synchronize()
    assert torch.equal(_i16(hbuf.cpu()), _i16(want_h.reshape(-1))), "h rows"
    assert torch.equal(ssbuf.cpu(), want_ss), (ssbuf.cpu()[:R, :16], want_ss[:R, :16])


@pytest.mark.parametrize("Hd", [8, 2560, 4096])
def test_embed_rows_single(ops, tables, Hd):
    emb = tables[Hd]
    for n in (16, 0, 7, 1):
        ids = torch.randint(0, 1000, (24,), generator=H.gen(n + Hd))
        ids[0], ids[n - 1] = 0, 999
        dyn = sent((8,), 5000, I32)
        dyn[RR.BS] = n
        hbuf = torch.full((16 * Hd + 64,), float("nan"), dtype=BF16).to(dev())
        ssbuf = sent((24,), 100).to(F32).to(dev())
        ops.embed_rows(emb.to(dev()), ids.to(dev()), hbuf, Hd, ssbuf, dyn.to(dev()), RR.BS)
        want_h = torch.full((16 * Hd + 64,), float("nan"), dtype=BF16)
        want_ss = sent((24,), 100).to(F32)
        rows = emb[ids[:n]]
        want_h[:n * Hd] = rows.reshape(-1)
        want_ss[:16] = 0
        want_ss[:n] = rows.double().pow(2).sum(-1).float()
        torch.cuda.synchronize()
        assert torch.equal(_i16(hbuf.cpu()), _i16(want_h)), f"h rows, count {n}"
        assert torch.equal(ssbuf.cpu(), want_ss), f"ss, count {n}"


# ---- i. dfl_prefill_pack_rows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 8192, 8224, 20480])
def test_prefill_pack_rows(ops, K):
    """K = 8224: one full column chunk plus one k-step; 20480: the 8B draft's fc_in.  Rows of stride K + 8 into a
    NaN-filled tile buffer: rows < P bit-equal, every fragment of the padded rows zero, nothing past the tiles."""
    for P in (1, 127, 128, 129, 300):
        Pp = ops.prefill_rows_padded(P)
        assert Pp == (P + 127) // 128 * 128
        rows = (torch.randn(P, K + 8, generator=H.gen(P + K)) * 3).to(BF16)
        xf = torch.full((Pp * K + 64,), float("nan"), dtype=BF16).to(dev())
        ops.prefill_pack_rows(rows.to(dev())[:, :K], P, K, xf)
        torch.cuda.synchronize()
        got = xf.cpu()
        full = _i16(H.unpack_tiles(got[:Pp * K], Pp, K))
        assert torch.equal(full[:P], _i16(rows[:, :K])), f"P={P}: rows differ"
        assert not full[P:].any(), f"P={P}: padded rows are not zero"
        assert got[Pp * K:].isnan().all(), f"P={P}: written past the tiles"


# ---- j. dfl_argmax off the 16-byte-aligned path -------------------------------------------------------------------
def test_argmax_unaligned_rows_and_ties(ops):
    """Odd V leaves every row but the first unaligned (scalar path); row 0 takes the vector path with a scalar tail.
    Ties across the vector / scalar seam and across the 256-thread stride, an all-equal and an all -inf row."""
    g = H.gen(77)
    V = 151937
    x = torch.randn(3, V, generator=g).to(BF16)
    x[0, V - 2] = x[0, V - 1] = 9.0                      # last vector element and the scalar tail: the first wins
    x[1, 4000 + 256] = x[1, 4000] = x[1, 4000 + 512 + 3] = 9.0   # the same thread one and two strides on, and another
    x[2, V - 1] = 9.0                                    # the very last column of an unaligned row
    small = torch.randn(4, 5, generator=g).to(BF16)
    small[0] = 1.5                                       # all equal -> 0
    small[1] = float("-inf")                             # all -inf -> 0
    small[2, 1] = small[2, 4] = 7.0
    f = torch.randn(3, 1003, generator=g)
    f[0, 1000] = f[0, 999] = 50.0                        # fp32: vector part ends at 1000
    f[1, 300 + 256] = f[1, 300] = 50.0
    f[2] = float("-inf")
    f[2, 1002] = -1e30
    for name, t, want in (("bf16 wide", x, [V - 2, 4000, V - 1]), ("bf16 small", small, [0, 0, 1, None]),
                          ("fp32", f, [999, 300, 1002])):
        got = ops.argmax(t.to(dev())).cpu()
        ref = torch.argmax(t.float(), dim=-1)
        assert got.tolist() == ref.tolist(), name
        for gi, w in zip(got.tolist(), want):
            assert w is None or gi == w, (name, got.tolist(), want)
