"""Plain-Python model of the integer records that steer a decode cycle, written from include/dflash_hip.h and the
reference loop (model/dflash.py:258-268), not from the kernels: acceptance scan, commit, stop test, the length records
of the single, batch and per-tile forms, the re-armed block, slot admission and the two setters.

Everything is ints and lists, mutated in place: a test copies a device buffer to nested lists (`tensor.tolist()`),
applies these functions and compares the WHOLE lists with what the kernel left.  A record is an 8-int list; a "row"
is one request's slice of a 2-D buffer, at its full stride, so words a kernel must not touch stay in the comparison.
"""

WORDS = 8
S, TAU, BS, POS0, START, STOP, CYCLE = range(7)      # include/dflash_hip.h DFL_DYN_*; word 7 is spare


def clamp(x, lo, hi):
    return lo if x < lo else hi if x > hi else x


def accept(block, post, bs, start, out, out_len, stops):
    """model/dflash.py:258-261 for one request: acc = number of leading i < bs - 1 with block[i + 1] == post[i]; the
    tokens block[0..acc] + [post[acc]] go to out[start + i] where start + i < out_len.  hit: any of those acc + 2 tokens
    is a stop id, clipped or not.  Returns (acc, new_start, hit)."""
    acc = 0
    while acc < bs - 1 and block[acc + 1] == post[acc]:
        acc += 1
    toks = list(block[:acc + 1]) + [post[acc]]
    for i, t in enumerate(toks):
        if start + i < out_len:
            out[start + i] = t
    return acc, start + acc + 1, any(t in stops for t in toks)


def rearm(row, bonus, mask_id, n):
    """The next cycle's block: [bonus token, mask ids] over n slots (model/dflash.py:235); the rest of the row stays."""
    for i in range(n):
        row[i] = bonus if i == 0 else mask_id


# ---- single form (dfl_accept_commit: plain, re-arm, dyn_t) ------------------------------------------------------
def single_dyn(dyn, start, acc, hit):
    dyn[S], dyn[TAU], dyn[POS0], dyn[START] = start, acc + 1, start, start + acc + 1
    dyn[STOP] |= int(hit)
    dyn[CYCLE] += 1


def single_dyn_t(dyn_t, new_start):
    """_rearm_t's block-form record of the next verify; BS, STOP, CYCLE and word 7 are left alone."""
    dyn_t[S] = dyn_t[POS0] = dyn_t[START] = new_start
    dyn_t[TAU] = 0


def single_cycle(block, post, bs, out, out_len, dyn, stops, result=None, next_block=None, rearm_n=0, mask_id=0,
                 dyn_t=None):
    """One dfl_accept_commit* launch.  next_block may be `block` itself (re-arm in place)."""
    start = dyn[START]
    acc, new_start, hit = accept(block, post, bs, start, out, out_len, stops)
    bonus = post[acc]
    single_dyn(dyn, start, acc, hit)
    if dyn_t is not None:
        single_dyn_t(dyn_t, new_start)
    if result is not None:
        result[0:4] = [acc, new_start, dyn[STOP], dyn[CYCLE]]
    if next_block is not None:
        rearm(next_block, bonus, mask_id, rearm_n)
    return acc


# ---- batch form (dfl_accept_commit_batch, _batch_t) ------------------------------------------------------------
def batch_records(dyn_d, dyn_t, result, start, bs, acc, hit):
    """Per-request records of the batch form: dyn_d as the single form; dyn_t the block form of the next cycle with
    BS, STOP and CYCLE mirrored; word 7 of both untouched."""
    single_dyn(dyn_d, start, acc, hit)
    new_start = start + acc + 1
    dyn_t[S] = dyn_t[POS0] = dyn_t[START] = new_start
    dyn_t[TAU], dyn_t[BS], dyn_t[STOP], dyn_t[CYCLE] = 0, bs, dyn_d[STOP], dyn_d[CYCLE]
    if result is not None:
        result[0:4] = [acc, new_start, dyn_d[STOP], dyn_d[CYCLE]]


def tile_records(dd, dt, j, start, bs, acc):
    """Tile j of a request: its share of the acc + 1 context rows and of the bs block rows.  Words not named are left
    as they were (park, set_block_size and admit own them)."""
    new_start = start + acc + 1
    dd[S] = dd[POS0] = start + 16 * j
    dd[TAU] = clamp(acc + 1 - 16 * j, 0, 16)
    dd[START] = new_start
    dt[S] = dt[POS0] = dt[START] = new_start
    dt[TAU] = 0
    dt[BS] = clamp(bs - 16 * j, 0, 16)


def batch_cycle(R, block, post, out, out_len, dyn_d, dyn_t, stops, result=None, next_block=None, mask_id=0,
                tiles_per_req=1, dyn_dt=None, dyn_tt=None):
    """One dfl_accept_commit_batch launch (dyn_dt None: no tile records) over requests 0..R-1.  block, post,
    out, next_block: lists of rows; dyn_*: lists of records (dyn_dt / dyn_tt: tiles_per_req per request; they may be
    dyn_d / dyn_t themselves at tiles_per_req = 1, as the batched decoder passes them).  bs = dyn_d[r][BS]; a request
    with bs == 0 is idle: no word of its slot changes.  Returns the accepted lengths (None for idle requests)."""
    accs = []
    for r in range(R):
        bs, start = dyn_d[r][BS], dyn_d[r][START]
        if bs == 0:
            accs.append(None)
            continue
        acc, new_start, hit = accept(block[r], post[r], bs, start, out[r], out_len, stops)
        bonus = post[r][acc]
        batch_records(dyn_d[r], dyn_t[r], result[r] if result is not None else None, start, bs, acc, hit)
        if dyn_dt is not None:
            for j in range(tiles_per_req):
                tile_records(dyn_dt[r * tiles_per_req + j], dyn_tt[r * tiles_per_req + j], j, start, bs, acc)
        if next_block is not None:
            rearm(next_block[r], bonus, mask_id, 16 * tiles_per_req)
        accs.append(acc)
    return accs


# ---- slot admission (dfl_admit_slot) ----------------------------------------------------------------------------
def admit(prompt, first, out_row, out_len, block_row, post_row, blk_w, result_row, n_tail, dyn_d, dyn_t, bs, mask_id,
          seeds=None, r=0, seed=0):
    """Every word dfl_admit_slot's header comment lists, for one slot's rows.  Returns which tail row each of the 16
    rows of the slot's context tile holds (None: a zero row)."""
    P = len(prompt)
    for i in range(out_len):
        out_row[i] = prompt[i] if i < P else first if i == P else mask_id
    for i in range(blk_w):
        block_row[i] = first if i == 0 else mask_id
        post_row[i] = 0
    result_row[0:4] = [0, 0, 0, 0]
    dyn_d[0:WORDS] = [P - n_tail, n_tail, bs, P - n_tail, P, 0, 0, 0]
    dyn_t[0:WORDS] = [P, 0, bs, P, P, 0, 0, 0]
    if seeds is not None:
        seeds[r] = seed
    return [i if i < n_tail else None for i in range(16)]


# ---- setters (dfl_set_dyn, dfl_set_dyn2) ------------------------------------------------------------------------
def set_dyn(rec, s, tau, bs, pos0):
    """{S, tau, bs, pos0, start = pos0 + tau, stop = 0, cycle = 0} and the spare word cleared."""
    rec[0:WORDS] = [s, tau, bs, pos0, pos0 + tau, 0, 0, 0]


def set_dyn2(recs, s, tau, bs, pos0):
    """Two records, tile t's with tau and bs clamped to its share; START = pos0 + tau unclamped in both."""
    for t in range(2):
        recs[WORDS * t:WORDS * (t + 1)] = [s, clamp(tau - 16 * t, 0, 16), clamp(bs - 16 * t, 0, 16), pos0, pos0 + tau,
                                           0, 0, 0]
