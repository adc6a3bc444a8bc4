"""The host segmenter and the host folding over every Unicode scalar value (no GPU).

fac_segment_graphemes against regex \\X in the eight contexts of unicode_contexts (1 112 064 lines
each, nothing sampled), fac_fold_first_char against str.lower() for every scalar value, and the
generated lowercase table against str.lower() in full. These guard against a stale
unicode_data.inc; the device lookups of the same tables are checked by test_gpu_unicode_exhaustive."""
import ctypes
import os
import re

import numpy as np
import pytest

import unicode_contexts as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_u64p = ctypes.POINTER(ctypes.c_uint64)


def host_starts(data: bytes):
    from fuzzy_aho_corasick import _native
    out = np.zeros(len(data) + 1, dtype=np.uint64)
    n = _native.lib.fac_segment_graphemes(data, len(data), out.ctypes.data_as(_u64p), len(out))
    return out[: int(n)]


@pytest.mark.parametrize("k", range(len(U.CONTEXTS)), ids=U.CONTEXT_IDS)
def test_host_segmentation_of_every_scalar_value(k):
    pre, post, _ = U.CONTEXTS[k]
    ctx = U.ContextText(pre, post)
    assert len(ctx.cps) == 1_112_064
    U.check_starts(ctx, host_starts(ctx.data))


def test_host_segmentation_at_start_and_end_of_text():
    """The class representatives (lowest and highest code point of every property triple per tier) as
    a whole text's first code point and as its last: seg_init and the text's end."""
    reps = U.class_representatives()
    assert 40 <= len(reps) <= 200
    for pre, post, _ in U.CONTEXTS:
        for cp in reps:
            for text in (chr(cp) + post, pre + chr(cp)):
                want, _ = U.expected(text)
                assert host_starts(text.encode()).tolist() == want.tolist(), (hex(cp), pre, post)


def test_host_first_char_folding_of_every_scalar_value():
    """fac_fold_first_char = lower_full's first code point; the only host route to lower_full (a
    pattern's full folded form is built with the engine, which needs a device: the device tests
    compare it through the symbol ids)."""
    from fuzzy_aho_corasick import _native
    fold = _native.lib.fac_fold_first_char
    low = U.lower_first_table()
    bad = []
    for cp in U.ALL_SCALARS.tolist():
        b = chr(cp).encode("utf-8")
        if fold(b, len(b), 1) != low[cp] or fold(b, len(b), 0) != cp:
            bad.append(f"U+{cp:04X} ({U.tier(cp)}): folds to U+{fold(b, len(b), 1):04X}, expected U+{int(low[cp]):04X}; "
                       f"unfolded U+{fold(b, len(b), 0):04X}")
            if len(bad) >= 5:
                break
    assert not bad, bad


def test_generated_lowercase_table_is_str_lower():
    """kLowerMap of unicode_data.inc, read as data: exactly the code points whose str.lower() differs
    from them, each with its full mapping (U+0130 has two code points), in ascending order."""
    src = open(os.path.join(REPO, "fuzzy-aho-corasick-rs_amd", "csrc", "unicode_data.inc")).read()
    body = src[src.index("kLowerMap[]"):]
    body = body[: body.index("};")]
    rows = re.findall(r"\{0x([0-9A-Fa-f]+), \{0x([0-9A-Fa-f]+), 0x([0-9A-Fa-f]+), 0x([0-9A-Fa-f]+)\}, (\d)\}", body)
    table = {int(c, 16): [int(x, 16) for x in (a, b, d)][: int(n)] for c, a, b, d, n in rows}
    assert [int(r[0], 16) for r in rows] == sorted(table)
    cased = U.cased_code_points()
    assert sorted(table) == cased and len(cased) == 1393
    for cp in cased:
        assert table[cp] == [ord(c) for c in chr(cp).lower()], hex(cp)
    assert table[0x130] == [0x69, 0x307] and sum(cp >= 0x10000 for cp in cased) == 225
