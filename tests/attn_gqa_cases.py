"""Case tables of tests/test_hip_attn_gqa.py: every attention entry point across GQA group sizes G = n_q / n_kv, at the
smallest shapes that reach each G-dependent rule of csrc/attn_head.hip, csrc/attn_block.hip and csrc/prefill.hip.  No GPU
and no dflash_amd.ops here: tests/test_attn_keys_cpu.py asserts, without a GPU, what the tables promise (every case has
n_kv >= 2, which groups reach which entry point, which launch form each dfl_attn_head case gets), so an edit that drops a
group fails a CPU test.

Why n_kv >= 2 everywhere: head = kvh * G + hh; with one kv head kvh * G is 0 whatever G is.  Every needle launch probes
every head of every kv group (attn_keys_ref.needle_problem), so a kv group >= 1 is probed as soon as there is one."""
import attn_keys_ref as R

# groups dfl_attn_head and its forms take beyond {2, 4}: MHA, the odd ones, an even non-power-of-two, 8 and 16
GROUP_HEADS = {1: (2, 2), 3: (6, 2), 5: (10, 2), 6: (12, 2), 7: (14, 2), 8: (16, 2), 16: (32, 2)}
ODD_HEADS = [GROUP_HEADS[g] for g in (3, 5, 6)]          # the groups every form below runs


def group(heads) -> int:
    return heads[0] // heads[1]


# ---------------------------------------------------------------- dfl_attn_head, single request
# (n_q, n_kv, S, tau, bs, max_splits, q_tiles, dyn bound or None) as tests/test_hip_attn_keys.HEAD_CASES
HEAD_SHORT = [(n_q, n_kv, S, tau, 16, 8, 1, bound) for n_q, n_kv in GROUP_HEADS.values() for S, tau in ((33, 0), (1041, 16))
              for bound in (None, S)]
HEAD_LONG = [(12, 2, 5300, 0, 16, 32, 1, None), (12, 2, 5300, 7, 16, 32, 1, 5300), (16, 2, 5300, 0, 16, 32, 1, None),
             (40, 8, 5300, 0, 16, 32, 1, None)]
HEAD_QT2 = [(n_q, n_kv, 70, tau, bs, 8, 2, None) for n_q, n_kv in ((10, 2), (12, 2)) for bs in (17, 32) for tau in (0, 32)]
HEAD_CASES = HEAD_SHORT + HEAD_LONG + HEAD_QT2


def head_form(c) -> dict:
    n_q, n_kv, S, tau, bs, ms, qt, bound = c
    return R.head_form(n_q, n_kv, S if bound is None else bound, bs, ms, q_tiles=qt, dyn=bound is not None)


def head_id(c) -> str:
    n_q, n_kv, S, tau, bs, ms, qt, bound = c
    f = head_form(c)
    return (f"G{n_q // n_kv}-({n_q},{n_kv})-S{S}-tau{tau}-bs{bs}-{'imm' if bound is None else f'dyn{bound}'}-"
            f"{f['kernel']}-ns{f['ns']}-tpw{f['tiles_per_wave']}")


# ---------------------------------------------------------------- dfl_attn_head_batch / _batch_f32
# name: (form, heads, lens, bss, cache rows = kv_len_max).  One request at S = 0 in every case.  (12, 2) at R = 4 needs
# ~1100 keys for the pair rule (nt > 8 splits' worth of tiles with 256 / (12 * 4) - 1 = 4 splits): it gets its own lengths.
LENS4, LENS2 = (300, 0, 17, 600), (0, 600)
BATCH_CASES = {}
for _form in ("f32", "bf16"):
    for _heads in ODD_HEADS:
        _long = _heads == (12, 2)
        BATCH_CASES[f"{_form}-R4-G{group(_heads)}"] = (_form, _heads, (300, 0, 17, 1150) if _long else LENS4,
                                                        (16, 16, 5, 12), 1200 if _long else 700)
        BATCH_CASES[f"{_form}-R2-G{group(_heads)}"] = (_form, _heads, LENS2, (16, 9), 700)
    BATCH_CASES[f"{_form}-R4-G5-40x8"] = (_form, (40, 8), LENS4, (16, 7, 16, 12), 700)


def batch_form(name) -> dict:
    """attn_head_launch's rule for a ragged-batch launch: sized for kv_len_max - 16 cached keys, R blocks per launch."""
    _, (n_q, n_kv), lens, _, rows = BATCH_CASES[name]
    return R.head_form(n_q, n_kv, rows - 16, 16, 32, n_cand=len(lens), dyn=True)


def batch_id(name) -> str:
    f = batch_form(name)
    return f"{name}-{f['kernel']}-ns{f['ns']}-tpw{f['tiles_per_wave']}"


# ---------------------------------------------------------------- _cand, _oproj, block, fused, prefill
CAND_HEADS = ODD_HEADS                                     # C = 4 on a 300-key prefix
OPROJ_CASES = [(heads, S, tau) for heads in ODD_HEADS for S, tau in ((40, 0), (1100, 9))]       # H = 512
BLOCK_GROUPS = (1, 2, 3, 5, 7, 8)                          # dfl_block_attn takes 1..8; n_kv = 2
BLOCK_CASES = [(g, S, ms) for g in BLOCK_GROUPS for S in (33, 1000) for ms in (32, 2)]
BLOCK_REFUSED = (18, 2)                                    # G = 9
FUSED_HEADS = [(2, 2), (4, 2), (16, 2)]                    # dfl_attn_fused(_batch) takes G in {1, 2, 4, 8}; G = 4 at
FUSED_CASES = [(h, S, tau) for h in FUSED_HEADS for S, tau in ((41, 5), (1100, 0))]   # n_kv = 2 is test_hip_attn_keys'
FUSED_REFUSED = [(6, 2), (10, 2), (12, 2), (14, 2), (32, 2)]                          # G = 3, 5, 6, 7, 16
PREFILL_HEADS = [(6, 2), (10, 2), (12, 2), (14, 2), (16, 2), (32, 2)]
PREFILL_P = (17, 45, 300)


def prefill_form(heads) -> tuple:
    """dfl_prefill_attn: (query heads per workgroup, workgroups per kv head)."""
    g = group(heads)
    hq = 4 if g % 4 == 0 else 2 if g % 2 == 0 else 1
    return hq, g // hq


ROW_HEADS = [(6, 2), (10, 2), (16, 2)]                     # the row stages that carry head counts


def all_heads() -> list:
    """Every (n_q, n_kv) any table above launches."""
    hs = [c[:2] for c in HEAD_CASES] + [v[1] for v in BATCH_CASES.values()] + CAND_HEADS + [c[0] for c in OPROJ_CASES]
    hs += [(2 * g, 2) for g in BLOCK_GROUPS] + [BLOCK_REFUSED] + FUSED_HEADS + FUSED_REFUSED + PREFILL_HEADS + ROW_HEADS
    return sorted(set(hs))
