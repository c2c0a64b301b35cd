"""CPU only: the data of tests/test_gpu_paged_long_context.py tells the faults of a paged decoder apart.  For every case of that file the step
(or the prompt pass) is restated from oracle primitives over the loaded rows, and four wrong versions of it -- (a) row T - 1 an ordinary row,
(b) the slab's poison row behind the new rows attended, (c) the middle split's chunk lost, for every plan the case runs, (d) the first marked
interior page replaced by the same page of another sequence -- must each MISS the bound the product is held to against the oracle, while the
unmodified restatement meets it.  Sequences without an interior page or a second split (70 positions, the fillers) take (a) and (b).  The token
checks of the GPU file are "margin permitting": at least half of the compared (row, step) pairs are decided by the oracle's margin."""
import numpy as np
import pytest

from tests import test_gpu_paged_long_context as plc
from tests._util import assert_vec_close

G = plc.G
# (geometry, sequence, regime, plans [(attended, splits)], the sequence whose page replaces one): the single-sequence decoder (regime 6), the rows of
# the unequal batch below 6 rows (6) and from 6 rows and in the mixed pass (1); 32 splits at B = 3, 5, 6 and in the mixed pass, 8 at B = 33
P = plc.STEP_PLANS
STEP_CASES = [
    (G, "d", 6, P["d"], "c"),
    (G, "c", 6, P["c"][:1], "a"),
    (G, "a", 6, P["a"][:1], "c"),
    ("r8d64", "c", 6, P["c"][:1], "m"),
    (G, "a", 1, P["a"], "c"),
    (G, "c", 1, P["c"], "a"),
    (G, "b", 6, [], None), (G, "b", 1, [], None), (G, "f0", 6, [], None), (G, "f0", 1, [], None),
]
# (sequence, L, the other sequence): test 2's suffixes, then the chunk and the forked suffixes of the mixed pass
SUFFIX_CASES = [(n, L, "a") for n, L in plc.SUFFIXES] + [("m", 40, "a"), ("c", 7, "a"), ("c", 70, "a")]


def must_miss(got, want, dt, what):
    with pytest.raises(AssertionError):
        assert_vec_close(got, want, dt, what=what)


@pytest.mark.parametrize("geom,name,regime,plans,other", STEP_CASES, ids=lambda x: x if isinstance(x, str) else None)
def test_step_restatement_variants_miss_the_bound(geom, name, regime, plans, other):
    dt = plc.GEOM[geom][1]
    want = plc.oracle_steps(geom, name, regime)[0]
    assert_vec_close(plc.restated_step(geom, name, regime), want, dt, what="the unmodified restatement")
    variants = ["marker", "poison"] + [("split",) + p for p in plans] + ([("page", other)] if other else [])
    for v in variants:
        must_miss(plc.restated_step(geom, name, regime, v), want, dt, f"{geom} {name} regime {regime} variant {v}")


@pytest.mark.parametrize("name,L,other", SUFFIX_CASES)
def test_suffix_restatement_variants_miss_the_bound(name, L, other):
    dt, T = plc.GEOM[G][1], plc.SEQ_T[name]
    want = plc.oracle_suffix(G, name, L)[0]
    assert_vec_close(plc.restated_suffix(G, name, L), want, dt, what="the unmodified restatement")
    for v in ("marker", "poison", ("split", T + L + 1, 32), ("page", other)):
        must_miss(plc.restated_suffix(G, name, L, v), want, dt, f"{name} L={L} variant {v}")


I8_CASES = [(G, "a", 6, P["a"][:1], "c"), (G, "c", 6, P["c"][:1], "a"), (G, "a", 1, P["a"][:1], "c"), (G, "c", 1, P["c"][:1], "a"),
            (G, "b", 6, [], None), (G, "b", 1, [], None), (G, "f0", 1, [], None),
            ("r8d128", "a", 6, P["a"][:1], "c"), ("r8d128", "c", 6, P["c"][:1], "a"), ("r8d128", "b", 6, [], None)]


@pytest.mark.parametrize("geom,name,regime,plans,other", I8_CASES, ids=lambda x: x if isinstance(x, str) else None)
def test_int8_restatement_variants_miss_the_bound(geom, name, regime, plans, other):
    """The same on int8 pages (32 splits at B = 3 and 8): every variant's rows quantised with the pool's scales, the poison row code 127; the
    reference is the restatement itself, which models the quantisation exactly."""
    dt = plc.GEOM[geom][1]
    want = plc.i8_steps(geom, name, regime)[0][0]
    assert np.array_equal(plc.restated_step(geom, name, regime, i8=True), want)
    for v in ["marker", "poison"] + [("split",) + p for p in plans] + ([("page", other)] if other else []):
        must_miss(plc.restated_step(geom, name, regime, v, i8=True), want, dt, f"int8 {geom} {name} regime {regime} variant {v}")


def test_plans_restated_from_the_code():
    """batch_attn_splits and plan_attention at the shapes the GPU file runs."""
    assert [plc.batch_splits(B, 512, 2) for B in (2, 3, 5, 6, 33)] == [32, 32, 32, 32, 8]
    assert [plc.batch_splits(B, 4, 2) for B in (1, 2, 3, 5, 6, 29, 33)] == [1, 1, 1, 1, 32, 4, 1]
    assert [plc.decoder_splits(c, 2) for c in (1024, 2048, 4160, 32768, 65536)] == [4, 32, 32, 32, 32] and plc.decoder_splits(4160, 1) == 32


def test_markers_sit_where_the_cases_cut():
    """Markers on both sides of every split boundary of every plan, of two interior page boundaries, at rows 0, T - 1 and 8191 / 8192."""
    from tests._util import split_edges
    cuts = [(geom, name, [(t + st, s) for t, s in plans for st in range(plc.N_ORC)]) for geom, name, _, plans, _ in STEP_CASES]
    cuts += [(G, n, [(plc.SEQ_T[n] + L + k, 32) for L in plc.SUFFIX_L[n] for k in range(3)]) for n in "pqm"]   # the suffix's last row and two steps behind it
    for geom, name, plans in cuts:
        T = plc.SEQ_T[name]
        k = plc.seq_layers(geom, name)[0][0][:, :T]
        norm = np.sqrt((k.astype(np.float64) ** 2).sum(-1)).min(0)          # the smaller kv-head's row norm
        marked = set(np.nonzero(norm > 3.0 * np.median(norm))[0].tolist())
        need = {0, T - 1} | {r for r in (8191, 8192) if r < T}
        for t, s in plans:
            need |= {r for r in split_edges(t, s) if r < T}
        for j in plc.page_markers(T):
            need |= {plc.PAGE * j - 1, plc.PAGE * j}
        assert need <= marked, (geom, name, sorted(need - marked)[:8])


def test_most_compared_tokens_are_decided_by_the_oracle():
    pairs = []
    for geom, name in [(G, "d"), (G, "c"), (G, "a"), ("r8d64", "c")]:
        pairs += [(v, plc.GEOM[geom][1]) for v in plc.oracle_steps(geom, name, 6)[:plc.STEPS1[name]]]
    for regime, names in ((6, "abc"), (6, ["a", "b", "c", "f0"]), (1, ["a", "b", "c", "f0"]), (1, ["a", "b", "c", "f0"])):   # B = 3, 5, 6, 33
        pairs += [(v, plc.BF) for n in names for v in plc.oracle_steps(G, n, regime)[:plc.STEPS]]
    for name, L in plc.SUFFIXES:
        first, _, steps = plc.oracle_suffix(G, name, L)
        pairs += [(v, plc.BF) for v in [first] + steps]
    pairs += [(v, plc.BF) for v in plc.oracle_mixed()]
    for geom, regime, names in ((G, 6, "abc"), (G, 1, ["a", "b", "c", "f0"]), ("r8d128", 6, "abc")):                       # int8 pages
        pairs += [(v, plc.BF) for n in names for v, _ in plc.i8_steps(geom, n, regime)]
    for v, _ in pairs:
        assert np.abs(v).max() > 0.5, "a reference logits vector is degenerate"
    n = sum(1 for v, dt in pairs if plc.decided(v, dt))
    assert 2 * n >= len(pairs), f"only {n} of {len(pairs)} compared (row, step) pairs have a decided greedy token"
