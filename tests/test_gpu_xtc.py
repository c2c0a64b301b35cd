"""-m gpu: the XTC op (pie_sample_xtc / pie_sample_rows_xtc), differentially: the token, the kept mask and the kept count
are those of today's pie_sample over a copy of the log-probabilities with the reference's removed set (tests/xtc_reference.py) at
-inf, on the same seed and counter; `removed` is the set's size; the coin is the Python Philox's.  Every comparison is exact."""
import math

import numpy as np
import pytest
import torch

from tests import xtc_reference as ref

pytestmark = pytest.mark.gpu

THR = 0.1
LT = ref.log_threshold(THR)
VOCABS = [1, 2, 511, 512, 513, 1537, 128256]
MODES = {"categorical": ("categorical", 0.9, 0.0, 0), "top_k": ("top_k", 0.8, 0.0, 5), "top_p": ("top_p", 1.0, 0.9, 0), "min_p": ("min_p", 0.7, 0.05, 3)}
L = lambda p: np.float32(math.log(p))


def mode_args(mode, V):
    name, temp, p, k = MODES[mode]
    if name == "top_k":
        k = min(k, V - 1)
    if name == "min_p":
        k = min(k, V)
    return name, temp, p, k


def base_row(V, seed):
    """fp32 values all at least half a nat below the threshold: no candidate of their own."""
    rng = np.random.default_rng(seed)
    return np.minimum((rng.standard_normal(V) * 2.0 - 6.0).astype(np.float32), np.float32(LT - 0.5))


def planted(V, seed=0):
    """Candidates at the first, the middle and the last id (as many as V holds): 0.5, 0.3, 0.15."""
    lp = base_row(V, seed)
    for i, p in zip(sorted({0, V // 2, V - 1}), (0.5, 0.3, 0.15)):
        lp[i] = L(p)
    return lp


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def check(lp, mode, threshold=THR, special=(), probability=1.0, seed=11, call=0, want_removed=None):
    """One call with XTC against pie_sample on the edited copy, same seed and counter.  Returns the reference's removed set."""
    from proxy_inference_engine_amd import hip_ops, samplers
    from proxy_inference_engine_amd.samplers import _rng
    V = lp.size
    args = mode_args(mode, V)
    yes = ref.coin(seed, call, probability)
    R = ref.removed_set(lp, threshold, special) if yes else np.zeros(V, bool)
    if want_removed is not None:
        assert int(R.sum()) == want_removed, (int(R.sum()), want_removed)   # the row bites as designed
    counter = _rng.hip_state(torch.device("cuda", torch.cuda.current_device()))[1]
    samplers.seed(seed)
    counter[0] = call
    tok, kept, mask, removed = hip_ops.sample(dev(lp), *args, want_mask=True, xtc=hip_ops.xtc_pack(probability, threshold, special), want_removed=True)
    after = counter.tolist()
    samplers.seed(seed)
    counter[0] = call
    tok0, kept0, mask0 = hip_ops.sample(dev(ref.edited(lp, R)), *args, want_mask=True)
    assert after == counter.tolist() == [call + 1, 0]                       # the call counter advances as without
    mask0 = mask0.cpu().numpy()[0].astype(bool)
    assert int(removed.item()) == int(R.sum())
    assert int(tok.item()) == int(tok0.item()) and not R[int(tok.item())]
    assert np.array_equal(mask.cpu().numpy()[0].astype(bool), mask0 & ~R)
    assert int(kept.item()) == int(kept0.item()) - int((mask0 & R).sum())
    return R


CASES = [(V, m) for V in VOCABS for m in MODES if not (V == 1 and m == "top_k")]   # (top_k needs 0 < k < V)


@pytest.mark.parametrize("V,mode", CASES)
def test_every_mode_and_size_equals_the_sampler_on_the_edited_copy(V, mode):
    R = check(planted(V, V), mode, want_removed=min(len({0, V // 2, V - 1}), 3) - 1 if V > 1 else 0)
    assert V < 3 or (R[0] and R[V // 2] and not R[V - 1])


def rows_1537():
    """name -> (lp, special, ids removed): each of the issue's designed rows at V = 1537 (three workgroups and one id more)."""
    V = 1537
    out = {}
    lp = base_row(V, 1)
    out["no candidate"] = (lp, (), [])
    lp = base_row(V, 2); lp[700] = L(0.4)
    out["one candidate"] = (lp, (), [])
    lp = base_row(V, 3); lp[3] = lp[700] = L(0.3)
    out["two tied"] = (lp, (), [])
    lp = base_row(V, 4); lp[3] = L(0.5); lp[600] = lp[1536] = L(0.2)
    out["two tied at the minimum of three"] = (lp, (), [3])
    lp = base_row(V, 5); lp[3] = L(0.2); lp[700] = L(0.6)
    out["two workgroups"] = (lp, (), [700])
    lp = base_row(V, 6); lp[5] = LT; lp[900] = L(0.5); lp[1200] = L(0.3)                 # lp == log_thr exactly: no candidate, and below the cut
    out["at the threshold exactly"] = (lp, (), [900])
    lp = base_row(V, 7); lp[4] = L(0.5); lp[513] = L(0.3); lp[1025] = L(0.15)
    out["a special id above the cut"] = (lp, (4, 5000, -1), [513])                      # (and two ids outside the vocabulary)
    out["all candidates special"] = (lp.copy(), (4, 513, 1025), [])
    lp = base_row(V, 8); lp[::2] = -np.inf; lp[1] = L(0.5); lp[701] = L(0.3); lp[1535] = L(0.12)
    out["-inf entries"] = (lp, (), [1, 701])
    lp = np.full(V, -np.inf, np.float32); lp[2] = L(0.5); lp[3] = L(0.3); lp[1000] = L(0.15); lp[1001] = L(0.04)
    out["top_k above the survivor count"] = (lp, (), [2, 3])                            # two finite survivors, top_k = 5
    return out


ROWS = rows_1537()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(ROWS))
def test_designed_rows(name, mode):
    lp, special, gone = ROWS[name]
    R = check(lp, mode, special=special, want_removed=len(gone))
    assert sorted(np.flatnonzero(R).tolist()) == gone


def test_min_p_refers_to_the_survivors_maximum():
    """p = {0.6, 0.2, 0.05, 0.03 x 5}, threshold 0.1, min_p 0.1: XTC removes id 0 alone, and the 0.03 ids pass min-p only against the
    survivors' maximum 0.2 (0.03 >= 0.02), not against 0.6 (0.03 < 0.06)."""
    from proxy_inference_engine_amd import hip_ops, samplers
    p = np.array([0.6, 0.2, 0.05] + [0.03] * 5)
    lp = np.full(513, -np.inf, np.float32)
    ids = [0, 100, 200, 300, 400, 500, 511, 512]
    lp[ids] = np.log(p).astype(np.float32)
    assert np.flatnonzero(ref.removed_set(lp, 0.1)).tolist() == [0]
    for seed in range(4):
        samplers.seed(seed)
        tok, kept, mask, removed = hip_ops.sample(dev(lp), "min_p", 1.0, 0.1, 1, want_mask=True, xtc=hip_ops.xtc_pack(1.0, 0.1), want_removed=True)
        assert ref.coin(seed, 0, 1.0)
        assert np.flatnonzero(mask.cpu().numpy()[0]).tolist() == ids[1:] and int(kept.item()) == 7 and int(removed.item()) == 1
        samplers.seed(seed)
        _, kept0, mask0 = hip_ops.sample(dev(lp), "min_p", 1.0, 0.1, 1, want_mask=True)                   # without XTC: 0.6 and 0.2 only
        assert np.flatnonzero(mask0.cpu().numpy()[0]).tolist() == ids[:2]
    check(lp, "min_p", want_removed=1)


@pytest.mark.parametrize("mode", list(MODES))
def test_probability_zero_is_off_and_a_null_record_is_the_old_op(mode):
    from proxy_inference_engine_amd import hip_ops, samplers
    lp = planted(1537, 9)
    args = mode_args(mode, 1537)
    samplers.seed(3)
    want = [t.cpu().numpy() for t in hip_ops.sample(dev(lp), *args, want_mask=True)]
    samplers.seed(3)
    off = hip_ops.sample(dev(lp), *args, want_mask=True, xtc=hip_ops.xtc_pack(0.0, THR), want_removed=True)
    samplers.seed(3)
    null = hip_ops.sample(dev(lp), *args, want_mask=True, want_removed=True)                               # pie_sample_xtc with a NULL record
    for got in (off, null):
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got[:3], want)) and int(got[3].item()) == 0
    check(lp, mode, probability=0.0, want_removed=0)
    check(lp, mode, probability=1.0, want_removed=2)


def test_the_coin_follows_the_python_philox_call_by_call():
    from proxy_inference_engine_amd import hip_ops, samplers
    lp, seed = dev(planted(1537, 10)), 0x1234_5678_9ABC_DEF1
    rec = hip_ops.xtc_records([hip_ops.xtc_pack(0.3, THR)], "cuda")
    samplers.seed(seed)
    flags = [int(hip_ops.sample(lp, "categorical", 1.0, xtc=rec, want_removed=True)[1].item()) for _ in range(64)]
    want = [2 if ref.coin(seed, call, 0.3) else 0 for call in range(64)]
    assert flags == want and 0 < sum(f > 0 for f in flags) < 64


def test_untrusted_record_bytes():
    """n_special beyond 16 acts as 16 (the words behind the record are never read as ids), a NaN probability or threshold removes nothing."""
    from proxy_inference_engine_amd import hip_ops, samplers
    lp = planted(1537, 11)
    rec = hip_ops.xtc_pack(1.0, THR, (0,))
    for n_special, prob, log_thr, removed in ((10 ** 6, 1.0, float(LT), 1), (-5, 1.0, float(LT), 2), (1, float("nan"), float(LT), 0), (1, 1.0, float("nan"), 0)):
        t = hip_ops.xtc_records([rec], "cuda")
        t[0, 2] = n_special
        t.view(torch.float32)[0, 0], t.view(torch.float32)[0, 1] = log_thr, prob
        samplers.seed(1)
        got = hip_ops.sample(dev(lp), "categorical", 1.0, xtc=t, want_removed=True)[1]
        assert int(got.item()) == removed, (n_special, prob, log_thr)


# ------------------------------------------------------------------ the rows form
def test_rows_form_equals_each_rows_own_call():
    """An off row, a greedy row (nothing of it written) and mixed records: row r equals its one-row call with counter {calls, 0}, wherever
    it sits and whoever its neighbours are."""
    from proxy_inference_engine_amd import hip_ops, samplers
    from proxy_inference_engine_amd.samplers import _rng
    V = 1537
    names = ["a special id above the cut", "two workgroups", "two tied at the minimum of three", "-inf entries", "at the threshold exactly", "no candidate"]
    specs = [  # (row_tail_pack arguments, xtc record arguments or None)
        (dict(mode="categorical", temp=0.9, seed=5, calls=3), (1.0, THR, (4,))),
        (dict(mode="top_k", temp=0.8, k=5, seed=6, calls=0), (0.0, THR, ())),                               # off
        (dict(mode=None), (1.0, THR, ())),                                                                  # greedy
        (dict(mode="top_p", temp=1.0, p=0.9, seed=7, calls=9), (1.0, THR, ())),
        (dict(mode="min_p", temp=0.7, p=0.05, k=3, seed=8, calls=2 ** 33), (0.5, THR, (900,))),
        (dict(mode="top_k", temp=1.2, k=4, seed=9, calls=1), (1.0, 0.05, ())),
    ]
    lps = [ROWS[n][0] for n in names]
    counter = _rng.hip_state(torch.device("cuda", torch.cuda.current_device()))[1]
    single = []
    for lp, (tail, xtc) in zip(lps, specs):
        if tail["mode"] is None:
            single.append(None)
            continue
        samplers.seed(tail["seed"])
        counter[0] = tail["calls"]
        out = hip_ops.sample(dev(lp), tail["mode"], tail["temp"], tail.get("p", 0.0), tail.get("k", 0), want_mask=True, xtc=hip_ops.xtc_pack(*xtc), want_removed=True)
        single.append([t.cpu().numpy()[0] for t in out])
    assert sum(int(s[3]) > 0 for s in single if s is not None) >= 3                                        # rows on which XTC did remove ids
    for order in ([0, 1, 2, 3, 4, 5], [5, 3, 0, 2, 4, 1]):
        table = hip_ops.row_tail_table([hip_ops.row_tail_pack(**specs[i][0]) for i in order], "cuda")
        xtc = hip_ops.xtc_records([hip_ops.xtc_pack(*specs[i][1]) for i in order], "cuda")
        tokens = torch.full((6,), -7, dtype=torch.int32, device="cuda")
        tok, kept, mask, removed = hip_ops.sample_rows(dev(np.stack([lps[i] for i in order])), table, tokens=tokens, want_mask=True, xtc=xtc, want_removed=True)
        removed = removed.cpu().numpy()
        for r, i in enumerate(order):
            if single[i] is None:
                assert int(tok[r].item()) == -7 and int(kept[r].item()) == 0 and not mask[r].any().item() and removed[r] == 0   # nothing written
                continue
            t0, k0, m0, r0 = single[i]
            assert (int(tok[r].item()), int(kept[r].item()), int(removed[r])) == (int(t0), int(k0), int(r0)), (order, r)
            assert np.array_equal(mask[r].cpu().numpy(), m0)
            calls = table[r, 3].item() & (2 ** 64 - 1)                                                     # (mode, inv_temp | thr, k | seed | calls)
            assert calls == specs[i][0]["calls"] + 1                                                       # the row's own counter advanced


def test_argument_checks():
    import ctypes as C
    from proxy_inference_engine_amd import _ffi, hip_ops
    lib = _ffi.load()
    lp = dev(planted(513, 1))
    rec = hip_ops.xtc_records([hip_ops.xtc_pack(1.0, THR)] * 2, "cuda")
    ws = hip_ops.sample_workspace(lp.device, 1, 513)
    counter = torch.zeros(2, dtype=torch.int64, device="cuda")
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    odd = C.c_void_p(rec.data_ptr() + 2)
    call = lambda x, rm=None: lib.pie_sample_xtc(_ffi.p(lp), 1, 513, 0, 1.0, 0.0, 0, 1, _ffi.p(counter), _ffi.p(ws), _ffi.p(tok), None, None, x, rm, _ffi.stream())
    assert call(odd) == -3 and call(_ffi.p(rec), odd) == -3 and call(_ffi.p(rec)) == 0 and call(None) == 0
    with pytest.raises(ValueError):
        hip_ops.sample(lp, "categorical", 1.0, xtc=rec[0, :5].contiguous())
    with pytest.raises(ValueError):
        hip_ops.sample_rows(lp[None], hip_ops.row_tail_table([hip_ops.row_tail_pack()], "cuda"), xtc=hip_ops.xtc_pack(1.0, THR))
    torch.cuda.synchronize()
