"""The engines and documents of the batch tests for engines with multi-character mappings
(test_gpu_batch_mappings.py on the device, test_batch_mappings_host.py on the oracle alone), pure
Python: random_batch of test_gpu_batch.py with one to three rules of the parity tests' MAP_RULES added
to the builder, and the hand-built document cuts."""
from oracle_harness import graphemes
from test_gpu_batch import Rng, random_batch
from test_gpu_parity import MAP_RULES, MAP_VOCAB_ASCII, MAP_VOCAB_UNI

# (seed, vocabulary): ASCII-only, Unicode and mixed; N_BATCHES batches each
DIFF_SEEDS = [(0x5EED_B001, MAP_VOCAB_ASCII), (0x5EED_B002, MAP_VOCAB_UNI),
              (0x5EED_B003, MAP_VOCAB_UNI + MAP_VOCAB_ASCII)]
N_BATCHES = 60


def mapping_batch(rng, vocab, allow_beam=True):
    """random_batch's engine and documents, one to three mapping rules (plain or scored, as in the
    parity tests) on the builder, and in every other document or so one side of each rule rewritten
    to its other side: random_batch writes a pattern into a document as it is spelt, so without the
    rewrite a mapping's two sides would meet only where two patterns happen to spell them."""
    b, pats, docs, thr = random_batch(rng, vocab, allow_beam)
    rules = []
    for _ in range(1 + rng.next() % 3):
        a, c = MAP_RULES[rng.next() % len(MAP_RULES)]
        score = [1.0, 0.8, 0.5][rng.next() % 3]
        b = b.mapping(a, c) if score == 1.0 else b.mapping_scored(a, c, score)
        rules.append((a, c))
    out = []
    for doc in docs:
        if rng.next() % 2:
            for a, c in rules:
                doc = doc.replace(a, c) if rng.next() % 2 else doc.replace(c, a)
        out.append(doc)
    return b, pats, out, thr


def words(pats):
    return [p if isinstance(p, str) else p.pattern for p in pats]


def mapping_only(row, doc: bytes, pattern: str) -> bool:
    """A record no edit explains: no insertion or deletion, yet the matched text and the pattern
    differ in their grapheme counts -- a mapping of unequal sides was taken."""
    s, e, ins, dele = row[0], row[1], row[4], row[5]
    return ins == 0 and dele == 0 and len(graphemes(doc[s:e].decode("utf-8"))) != len(graphemes(pattern))


# ---- the hand-built cuts: "ß" <-> "ss" and "æ" <-> "ae", edits 1
CUT_PATS = ["straße", "encyclopaedia", "groß"]
CUT_THR = 0.8


def cut_builder(B, L):
    return B().fuzzy(L().edits(1)).case_insensitive(True).mapping("ß", "ss").mapping("æ", "ae")


def pad(n, unit="ü"):
    """A document prefix of n graphemes that no pattern matches, non-ASCII."""
    return (unit + "q") * (n // 2) + ("z" if n % 2 else "")


def cut_batches():
    """name -> documents. A haystack side ("ss" for the pattern's "ß", "æ" for "ae") split by a
    document boundary, ending exactly at a document's last grapheme, and one grapheme short of it;
    Unicode -> ASCII, ASCII -> Unicode and Unicode -> empty -> Unicode neighbours; the batch's last
    document; documents of 256 and 257 graphemes."""
    return {
        # the side "ss" split: "...stras" | "se..." (ASCII | ASCII, Unicode | ASCII, Unicode | Unicode)
        "split_ss": ["die stras", "se ist", "ü stras", "se", "ü stras", "se ü", "ü stras", "", "se ü"],
        # the side "ss" of the pattern's last grapheme "ß" ends the document / the batch
        "ends_at_last": ["ü gross", "x", "ü gross", "ü encyclopædia", "", "ü gross", "ü strasse", "é gross"],
        # one grapheme short: the side would need the next document's first grapheme
        "one_short": ["ü gros", "s", "ü encyclop", "ædia", "ü stras", "se ü", "ü gros"],
        # neighbours: Unicode -> ASCII, ASCII -> Unicode, Unicode -> empty -> Unicode
        "neighbours": ["straße ü", "strasse", "strasse", "ü strasse", "gross ß", "", "", "ßtrasse encyclopædia"],
        # tile edges: the side "ss" at graphemes 254..255 of a 256-grapheme document, and of a 257 one
        "tile_256": [pad(249) + "strasse", "se", pad(249) + "strasse", pad(250) + "strasse", "e ü"],
        "tile_257": [pad(250) + "strasse", pad(251) + "stras", "se", pad(244) + "encyclopædia" + "ü"],
    }
