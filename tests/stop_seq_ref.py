"""A pure-Python model of dfl_stop_seq_rows (include/dflash_hip.h) and of the trim that follows it.

launch(): per slot the accepted length (the accept launch's ballot), the committed tokens, every window that ends on one
of them, the two conditions, the tie rule (smallest end, then smallest index) and the sticky hit record.  trim(): the
columns a finished request keeps — the earlier of the first stop id and the hit's end position."""
SEQS, SEQ_LEN, MAX_BS = 8, 16, 32
S_, TAU, BS, POS0, START, STOP, CYCLE = range(7)


def accepted(block, posterior, bs):
    """Leading i < bs - 1 with block[i + 1] == posterior[i]."""
    acc = 0
    while acc < bs - 1 and block[acc + 1] == posterior[acc]:
        acc += 1
    return acc


def committed(block, posterior, bs):
    """The ids of positions start + 1 .. start + acc + 1."""
    acc = accepted(block, posterior, bs)
    return list(block[1:acc + 1]) + [posterior[acc]]


def match(block, posterior, output_ids, start, bs, seqs, first_pos, min_end):
    """(e, k) of the winning match of one slot, or None.  seqs: a list of lists (an empty list: unused)."""
    new = committed(block, posterior, bs)

    def tok(p):
        if p <= start:
            return output_ids[p] if 0 <= p < len(output_ids) else -1
        return new[p - start - 1]

    for e in range(start + 1, start + len(new) + 1):          # the smallest end first
        for k, s in enumerate(seqs):                            # then the smallest index
            L = len(s)
            if L == 0 or e - L + 1 < max(first_pos, 0) or e < min_end:
                continue
            if all(tok(e - L + 1 + c) == s[c] for c in range(L)):
                return e, k
    return None


def launch(block, posterior, output_ids, dyn, tables, bs=None):
    """All slots, in place on dyn (a list of 8-word lists) and on every tables[s]["hit"].  tables[s]: dict(seqs, first_pos,
    min_end, hit).  bs None: the record's BS word, cut to 32 and to the rows' lengths."""
    for s, t in enumerate(tables):
        b = dyn[s][BS] if bs is None else bs
        b = min(b, MAX_BS, len(block[s]), len(posterior[s]))
        if b <= 0 or not any(len(q) for q in t["seqs"]):
            continue
        m = match(block[s], posterior[s], output_ids[s], dyn[s][START], b, t["seqs"], t["first_pos"], t["min_end"])
        if m is None:
            continue
        dyn[s][STOP] |= 1
        if t["hit"] == [-1, -1]:
            t["hit"] = [m[0], m[1]]


def trim(row, max_length, mask_id, stop_ids, n_in, hit=None, seq_lens=None, include=True):
    """(kept columns of `row`, index of the stop sequence that ended the request or None).  hit: [e, k] or None / [-1, -1];
    seq_lens: the lengths of the request's sequences."""
    cols = [c for c in range(min(max_length, len(row))) if row[c] != mask_id]
    cut_id = None
    if stop_ids:
        for j, c in enumerate(cols[n_in:]):
            if row[c] in stop_ids:
                cut_id = c
                break
    which = None
    last = cols[-1] if cols else -1
    if hit is not None and hit[0] >= 0 and hit[0] <= last and (cut_id is None or hit[0] <= cut_id):
        which = hit[1]
        keep_to = hit[0] if include else hit[0] - seq_lens[which]
        cols = [c for c in cols if c <= keep_to]
    elif cut_id is not None:
        cols = [c for c in cols if c <= cut_id]
    return cols, which
