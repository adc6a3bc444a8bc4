"""Template replacements and batched extraction, the parts that need no GPU: the entry points are
bound and exported, the Python fac_extract_args mirrors the header, the pure table helper
round-trips, and the template callback through the loop of matches.rs:170-187 gives the crate's own
documented result."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fac_replacements_create_templates", "fac_extract_batch", "fac_extract_batch_prefiltered"]


def test_entry_points_are_bound():
    from fuzzy_aho_corasick import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    header = open(os.path.join(REPO, "include", "fac.h")).read()
    for name in NAMES:
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\(" % name, header), name
    assert re.search(r"#define FAC_NO_INSERT UINT64_MAX\b", header)
    assert _native.FAC_NO_INSERT == 2 ** 64 - 1
    import fuzzy_aho_corasick as fac
    assert hasattr(fac, "Wrap") and hasattr(fac, "template_table")
    assert hasattr(fac.StagedBatch, "extract")
    for cls in (fac.FuzzyAhoCorasick, fac.Prefiltered):
        assert hasattr(cls, "matched_strings_batch") and hasattr(cls, "extract_batch"), cls
    assert hasattr(fac.FuzzyReplacer, "extract_batch")


def test_extract_args_layout_matches_header():
    """The Python fac_extract_args has the header's fields, in order, with the header's C types."""
    from fuzzy_aho_corasick import _native
    header = open(os.path.join(REPO, "include", "fac.h")).read()
    body = re.search(r"typedef struct fac_extract_args \{(.*?)\} fac_extract_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(.*?)(\w+)$", decl)
            fields.append((m.group(2), m.group(1).strip()))
    ctype = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64}
    size = 0
    align = 1
    offsets = {}
    for name, typ in fields:
        c = ctypes.c_void_p if typ.endswith("*") else ctype[typ]
        a = ctypes.alignment(c)
        offsets[name] = (size + a - 1) // a * a
        size = offsets[name] + ctypes.sizeof(c)
        align = max(align, a)
    size = (size + align - 1) // align * align
    assert [n for n, _ in fields] == [n for n, _ in _native.fac_extract_args._fields_]
    assert [n for n, _ in fields] == ["threshold", "order", "overlap", "unique_ids", "stream", "device_records",
                                      "device_record_cap", "device_doc_offsets", "device_text", "device_text_cap",
                                      "device_item_offsets"]
    assert ctypes.sizeof(_native.fac_extract_args) == size == 80
    for (name, typ), (_, c) in zip(fields, _native.fac_extract_args._fields_):
        want = ctypes.sizeof(ctypes.c_void_p) if typ.endswith("*") else ctypes.sizeof(ctype[typ])
        assert ctypes.sizeof(c) == want, name
        assert getattr(_native.fac_extract_args, name).offset == offsets[name], name


def test_wrap_is_a_small_value_type():
    from fuzzy_aho_corasick import Wrap
    w = Wrap("<b>", "</b>")
    assert (w.prefix, w.suffix) == ("<b>", "</b>") and w == Wrap("<b>", "</b>") and hash(w) == hash(Wrap("<b>", "</b>"))
    assert Wrap("[").suffix == ""
    assert w.render("x") == "<b>x</b>" and Wrap(b"\xc2\xab", "»").render("é") == "«é»"


@pytest.mark.parametrize("reps", [
    [],
    ["x"],
    [None],
    ["W"],          # replaced below by Wrap entries
    ["", None, "W", b"raw"],
    ["PJSC", "W", None, "«é»", "W", "W", None, "\0"],
])
def test_template_table_round_trips(reps):
    from fuzzy_aho_corasick import Wrap, _native, replacement_table, template_table
    wraps = [Wrap("**", "**"), Wrap("«é", "😀»"), Wrap("", "]"), Wrap("[", ""), Wrap("", ""), Wrap(b"<e>", b"</e>")]
    reps = [wraps[i % len(wraps)] if r == "W" else r for i, r in enumerate(reps)]
    data, offsets, keep, insert_at = template_table(reps)
    assert isinstance(data, bytes) and isinstance(keep, bytes)
    assert len(offsets) == len(reps) + 1 and offsets[0] == 0 and offsets[-1] == len(data)
    assert len(keep) == len(insert_at) == len(reps)
    raw = lambda x: x if isinstance(x, bytes) else x.encode("utf-8")  # noqa: E731
    for p, r in enumerate(reps):
        entry = data[offsets[p]:offsets[p + 1]]
        if isinstance(r, Wrap):
            k = insert_at[p]
            assert keep[p] == 0 and k == len(raw(r.prefix))  # in bytes, not characters
            assert entry[:k] == raw(r.prefix) and entry[k:] == raw(r.suffix)
            entry[:k].decode("utf-8"), entry[k:].decode("utf-8")  # both halves valid on their own
        else:
            assert insert_at[p] == _native.FAC_NO_INSERT
            assert (keep[p], entry) == ((1, b"") if r is None else (0, raw(r)))
    if not any(isinstance(r, Wrap) for r in reps):  # without a template: replacement_table's own answer
        assert (data, offsets, keep) == replacement_table(reps)


def test_template_table_rejects_other_types_and_leaves_replacement_table_alone():
    from fuzzy_aho_corasick import Wrap, replacement_table, template_table
    with pytest.raises(TypeError):
        template_table(["a", 3])
    with pytest.raises(TypeError):
        template_table([Wrap("a", 3)])
    with pytest.raises(TypeError):  # the 3-tuple helper does not know templates
        replacement_table([Wrap("a", "b")])


def splice(text, matches, callback):
    """matches.rs:170-187: `matches` are (start, end) in start order."""
    out, last = [], 0
    for s, e in matches:
        if s >= last:
            out.append(text[last:s])
            r = callback(text[s:e])
            out.append(text[s:e] if r is None else r)
            last = e
    out.append(text[last:])
    return "".join(out)


def test_template_callback_reproduces_the_crates_documented_example():
    """matches.rs:437-446: "ipsum and l0rem", the matches filtered to the one whose text contains
    "0", .replace(|m| Some(format!("**{}**", m.text))) == "ipsum and **l0rem**"."""
    from fuzzy_aho_corasick import Wrap
    text = "ipsum and l0rem"
    w = Wrap("**", "**")
    assert splice(text, [(10, 15)], w.render) == "ipsum and **l0rem**"
    # unfiltered, and the guard: a record that starts inside text already replaced contributes nothing
    assert splice(text, [(0, 5), (0, 0), (3, 8), (10, 15)], w.render) == "**ipsum** and **l0rem**"
    # an empty entry with the slot at 0 is "keep"
    assert splice(text, [(10, 15)], Wrap("", "").render) == splice(text, [(10, 15)], lambda t: None) == text
