"""Every entry point of include/dflash_hip.h is named by a bounds case (the COVERS table of a tests/test_hip_bounds_*.py
module, which points at an existing GPU test of that module), or is exempt because it launches nothing.  A new entry
point without a bounds case fails here."""
import glob
import importlib
import os
import re

import helpers as H

HEADER = os.path.join(H.ROOT, "include", "dflash_hip.h")
LAUNCHES_NOTHING = "launches nothing"
EXEMPT = {
    "dfl_version": LAUNCHES_NOTHING,
    "dfl_last_error": LAUNCHES_NOTHING,
    # size functions: plain host arithmetic
    "dfl_argmax_ws_bytes": LAUNCHES_NOTHING,
    "dfl_attn_ws_bytes": LAUNCHES_NOTHING,
    "dfl_attn_fused_ws_bytes": LAUNCHES_NOTHING,
    "dfl_attn_fused_batch_ws_bytes": LAUNCHES_NOTHING,
    "dfl_attn_head_ws_bytes": LAUNCHES_NOTHING,
    "dfl_gemm_batch_ws_bytes": LAUNCHES_NOTHING,
    "dfl_prefill_rows_padded": LAUNCHES_NOTHING,
    "dfl_prefill_moe_max_tiles": LAUNCHES_NOTHING,
    "dfl_prefill_moe_max_items": LAUNCHES_NOTHING,
    "dfl_batch_tiles": LAUNCHES_NOTHING,
    "dfl_batch_ksplit": LAUNCHES_NOTHING,
}


def entry_points():
    """The functions the header declares: `<type> dfl_name(` at the start of a line, outside the comments."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^(?:const char \*|int64_t |int )(dfl_\w+)\(", text, flags=re.M)
    assert len(names) == len(set(names)) and len(names) > 70, len(names)
    return names


def bounds_modules():
    mods = []
    for path in sorted(glob.glob(os.path.join(H.ROOT, "tests", "test_hip_bounds_*.py"))):
        mods.append(importlib.import_module(os.path.splitext(os.path.basename(path))[0]))
    assert len(mods) >= 5
    return mods


def test_every_entry_point_has_a_bounds_case_or_launches_nothing():
    covered = {}
    for m in bounds_modules():
        for name, test in m.COVERS.items():
            fn = getattr(m, test, None)
            assert callable(fn), f"{m.__name__}.COVERS[{name!r}] names {test!r}, which is no test of that module"
            marks = [mk.name for mk in getattr(fn, "pytestmark", [])]
            assert "gpu" in marks, f"{m.__name__}.{test} is not a GPU test"
            covered.setdefault(name, []).append(f"{m.__name__}.{test}")
    names = entry_points()
    assert set(EXEMPT.values()) == {LAUNCHES_NOTHING}, "the only admissible exemption: the entry point launches nothing"
    missing = [n for n in names if n not in covered and n not in EXEMPT]
    assert not missing, f"entry points without a bounds case: {missing}"
    stale = [n for n in list(covered) + list(EXEMPT) if n not in names]
    assert not stale, f"bounds cases / exemptions of entry points the header no longer declares: {stale}"
    both = [n for n in covered if n in EXEMPT]
    assert not both, both

