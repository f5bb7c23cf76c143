"""The logits-processing reference on the CPU (tests/logits_ref.py): the
condition on the shared inputs holds, a correct f32 kernel in any of three
summation orders stays inside the derived bounds, each named mutant of the
kernel violates a check, and the reference agrees with the CPU oracle
(orc.Oracle.process_logits) on the fixtures' vocabularies. No GPU."""
import numpy as np
import pytest

import logits_ref as lr
import orc

ORDERS = ("sequential", "chunked", "pairwise")


def test_inputs_cover_the_edges():
    """The shared inputs hold what the kernel tests rely on."""
    cs = {c.name: c for c in lr.cases()}
    assert {f"V{v}" for v in lr.VOCAB_SIZES} <= set(cs)
    assert all(c.R <= 64 and c.lc.n_vocab <= lr.MAX_VOCAB for c in cs.values())
    begs = {c.lc.beg for c in cs.values() if c.name.startswith("beg")}
    V = 3 * lr.LP_CHUNK + 100
    assert {lr.LP_CHUNK, lr.LP_CHUNK - 1, lr.LP_CHUNK + 1, 3 * lr.LP_CHUNK + 50, V} <= begs
    assert any(c.lc.beg == c.lc.eot + 1 for c in cs.values())
    states = {tuple(int(r[n]) for n in ("is_initial", "last_ts", "penult_ts", "has_ts"))
              for c in cs.values() for r in c.ctl}
    assert len(states) == 9
    temps = {float(r["temperature"]) for c in cs.values() for r in c.ctl}
    assert {0.0, 1.0} <= temps and len(temps) >= 4
    # every seek_delta class in written has_ts rows: 0, 1, 2, odd, the last
    # timestamp, beyond the end (the monotonic rule then kills every timestamp)
    for c in cs.values():
        if c.name.startswith("beg"):
            sds = lr._seek_deltas(c.lc.n_vocab, c.lc.beg)
            seen = {int(r["seek_delta"]) for r in c.ctl
                    if r["has_ts"] and r["active"] and r["sample"]}
            assert seen == set(sds), (c.name, seen)
            if c.lc.beg < c.lc.n_vocab:
                assert c.lc.beg + sds[5] // 2 > c.lc.n_vocab and sds[3] % 2 == 1
    # every max_initial_tid placement, and suppress_blank on and off, under a
    # written initial row; space and eot in different chunks
    initial = [c for c in cs.values()
               if any(r["is_initial"] and r["active"] and r["sample"] for r in c.ctl)]
    mit = {("off" if c.lc.max_initial_tid < 0 else "beg" if c.lc.max_initial_tid == c.lc.beg
            else "beg+50" if c.lc.max_initial_tid == c.lc.beg + 50
            else "last" if c.lc.max_initial_tid == c.lc.n_vocab - 1
            else "past" if c.lc.max_initial_tid > c.lc.n_vocab else "other") for c in initial}
    assert {"off", "beg", "beg+50", "last", "past"} <= mit, mit
    assert {c.lc.suppress_blank for c in initial} == {0, 1}
    assert any(c.lc.suppress_blank and c.lc.space_id // lr.LP_CHUNK != c.lc.eot // lr.LP_CHUNK
               for c in initial)
    # the argmax ties land where they are named, bit-equal and on top
    place = {n: (lr.tie_place(a), lr.tie_place(b)) for n, (a, b) in lr.TIE_PAIRS.items()}
    (ca, sa, wa, la), (cb, sb, wb, lb) = place["lanes"]
    assert (ca, sa, wa) == (cb, sb, wb) and la != lb
    (ca, sa, wa, la), (cb, sb, wb, lb) = place["waves"]
    assert (ca, sa) == (cb, sb) and wa != wb
    (ca, sa, wa, la), (cb, sb, wb, lb) = place["slots"]
    assert (ca, wa, la) == (cb, wb, lb) and sa != sb
    assert place["chunks"][0][0] != place["chunks"][1][0]
    assert place["chunks"][0][1:] == place["chunks"][1][1:]
    assert place["chunk_edge"][0][0] + 1 == place["chunk_edge"][1][0]
    for name, off in (("tie_text", 0), ("tie_ts", 0), ("tie_tid", lr.TIE_TID_OFF)):
        c = cs[name]
        for k, (a, b) in enumerate(list(lr.TIE_PAIRS.values())[:c.R]):
            r = lr.references(c)[k]
            sel = np.arange(c.lc.n_vocab) >= (c.lc.beg if name == "tie_tid" else 0)
            top = c.x[k][sel].max()
            assert c.x[k][off + a] == c.x[k][off + b] == top, (name, k)
            assert int((c.x[k][sel] == top).sum()) == 2
            assert r["rec"]["tid" if name != "tie_text" else "id"] == off + a
            if name == "tie_tid":   # the shifted pairs keep their kind
                pa, pb = lr.tie_place(off + a), lr.tie_place(off + b)
                kind = list(lr.TIE_PAIRS)[k]
                assert {"lanes": pa[:3] == pb[:3], "waves": pa[:2] == pb[:2] and pa[2] != pb[2],
                        "slots": pa[0] == pb[0] and pa[2:] == pb[2:] and pa[1] != pb[1],
                        "chunks": pa[0] != pb[0], "chunk_edge": True}[kind], (kind, pa, pb)
    for f in ("want_probs", "want_nosp", "active", "sample"):
        assert {int(r[f]) for c in cs.values() for r in c.ctl} == {0, 1}, f
    refs = [r for c in cs.values() for r in lr.references(c) if r["written"]]
    assert any(r["kill_text"] for r in refs) and any(not r["kill_text"] for r in refs)
    assert any((~r["kill"]).sum() == 1 for r in refs)
    assert any(r["rec"]["ptsum"] == 0 for r in refs)            # Sts = 0
    assert any(r["rec"]["id"] == len(r["kill"]) - 1 for r in refs)


def test_margin_condition_on_every_input():
    """Every discrete decision of every written row is settled by the
    reference alone (or is a constructed, bit-exact tie)."""
    for case in lr.cases():
        lr.check_margins(case)


@pytest.mark.parametrize("ulp", [0, 2, -2])
@pytest.mark.parametrize("order", ORDERS)
def test_emulation_inside_bounds(order, ulp):
    """A correct f32 kernel stays inside the bounds: each summation order,
    with expf / logf correctly rounded or 2 ulp off in either direction. The
    kernel's own order and the pairwise one are held to the kernel's bound
    (depth 37), the sequential one to the same formula with its own depth."""
    ratios = {}
    for case in lr.cases():
        depth = lr.sum_depth(order, case.lc.n_vocab)
        depth = lr.KERNEL_DEPTH if depth <= lr.KERNEL_DEPTH else depth
        refs = lr.references(case, depth)
        for k in range(case.R):
            got = lr.emulate(case.x[k], case.smask, case.ctl[k], case.lc, order, None, ulp)
            bad = lr.compare(refs[k], got, ratios)
            assert not bad, (case.name, k, bad)
    print(order, ulp, {k: round(v, 3) for k, v in ratios.items()})
    assert ratios and max(ratios.values()) <= 1.0


@pytest.mark.parametrize("mutant", lr.MUTANTS)
def test_mutant_is_caught(mutant):
    """A subtly wrong kernel violates a check on the shared inputs."""
    for case in lr.cases():
        refs = lr.references(case)
        for k in range(case.R):
            got = lr.emulate(case.x[k], case.smask, case.ctl[k], case.lc, "chunked", mutant)
            if lr.compare(refs[k], got):
                return
    pytest.fail(f"mutant {mutant} survives: the inputs or the bounds are too weak")


@pytest.mark.parametrize("arch", ["micro", "micro-v3"])
def test_reference_matches_the_oracle(make_model, arch):
    """Masks exactly, values within the bounds (the oracle sums sequentially
    in f32: the bound at that depth), for matching history and parameters."""
    o = orc.Oracle(make_model(arch))
    V, beg, eot = o.n_vocab, o.beg, o.eot
    sp, nst, space = lr.oracle_vocab(o)
    rng = np.random.default_rng(3)
    hists = [[], [17], [17, 900], [beg + 5], [beg], [beg + 5, 17], [beg + 5, 17, beg + 40],
             [beg + 5, 17, beg + 40, beg + 40], [beg, beg], [beg + 5, 17, beg + 40, beg + 40, 33]]
    params = [dict(), dict(suppress_nst=True), dict(no_timestamps=True), dict(tdrz=True),
              dict(bench_fixed_steps=4), dict(suppress_blank=False, max_initial_ts=0.0),
              dict(temperature=0.7, suppress_nst=True), dict(max_initial_ts=2.0)]
    ratios, fired = {}, set()
    for n, kw in enumerate(params):
        sm = lr.static_mask(V, sp, nst_ids=nst, **{k: v for k, v in kw.items()
                                                    if k in ("suppress_nst", "no_timestamps", "tdrz",
                                                             "bench_fixed_steps")})
        mi = kw.get("max_initial_ts", 1.0)
        lc = lr.LC(V, eot, beg, space, int(kw.get("suppress_blank", True)),
                   beg + int(round(mi / 0.02)) if mi > 0 else -1, o.nosp)
        for h, hist in enumerate(hists):
            # (no timestamp can have been sampled where all are suppressed;
            # a (text, ts) history would leave no id at all there)
            if (kw.get("bench_fixed_steps") or kw.get("no_timestamps")) and max(hist + [0]) >= beg:
                continue
            st = lr.ctl_of_history(hist, beg)
            c = dict(zip(lr.CTL.names, lr.ctl_row(temperature=kw.get("temperature", 0.0), **st)))
            x = rng.normal(0.0, 3.0, V).astype(np.float32)
            x[int(rng.integers(0, eot))] += 8.0
            x[beg:] += 3.0 * ((n + h) % 2)
            x = lr._settle(x, sm, c, lc)
            r = lr.reference(x, sm, c, lc, lr.sum_depth("sequential", V))
            lg, lp, pr, rec = o.process_logits(x, hist, bool(st["has_ts"]), st["seek_delta"], **kw)
            dead = ~np.isfinite(r["lp"])
            np.testing.assert_array_equal(np.isneginf(lg), dead, err_msg=f"{kw} {hist}")
            # the oracle's record carries the host's override for id >= beg
            want = dict(r["rec"])
            if want["id"] >= beg:
                want["tid"], want["pt"] = want["id"], want["p"]
                r["b_rec"]["pt"] = r["b_rec"]["p"]
            r["rec"] = want
            # (the oracle returns the logits after the mass rule: its text
            # entries are -inf under kill_text, the others are flt's)
            np.testing.assert_array_equal(lr.bits(lg)[~dead], lr.bits(r["flt"])[~dead])
            bad = lr.compare(r, (r["flt"], pr, lp, dict(zip(lr.REC, rec + (0.0,)))), ratios)
            assert not bad, (kw, hist, bad)
            fired.add(r["kill_text"])
    assert fired == {True, False}
    print(arch, {k: round(v, 3) for k, v in ratios.items()})
