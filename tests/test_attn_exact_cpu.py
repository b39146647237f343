"""The exact key-selection cases of tests/_attn_exact.py, without a GPU: every
case of both tables meets the four conditions on its reference (D1-D3 / P1-P3;
the fourth is that the loops below excuse nothing), holds the dark units the
rescale needs, the torch emulations of both kernels reproduce bf16(S / n) bit
for bit, and each mistake that can be switched on changes the output.

Which case cannot show which mistake:
  * wrong_gqa (head h reads kv head h % KVH): cases with one query head per kv
    head, where h % KVH is h // (H / KVH) for every h.  Every other case has
    KVH = 2 and shows it on each head whose mapping differs.
  * unscaled-l-trip / unscaled-o-trip: decode cases whose waves make a single
    trip per chunk (hd 64 with chunks of 128 keys: 32 keys a wave trip, 128 a
    block trip).  Nothing is rescaled inside their lane groups.
  * mask_shift = +1 in prefill: S = 1 with the cache ending at the prompt's
    last token.  There is no later key.
Everything else is asserted on every case.  The fixtures are module-scoped and
parametrised, so the tests run case by case and each case is built once.
"""
import pytest
import torch

import _attn_exact as AE
import _prefill_ref as PR

F64 = AE.F64


@pytest.fixture(scope="module", params=AE.DECODE_CASES, ids=AE.decode_id)
def dec(request):
    return AE.decode_inputs(request.param)


@pytest.fixture(scope="module", params=AE.PREFILL_CASES, ids=AE.prefill_id)
def pre(request):
    return AE.prefill_inputs(request.param)


def _all_positions(case):
    return AE.decode_positions(case.plan) + [case.ctx, case.ctx + 7]


# ---- the tables ------------------------------------------------------------------------

def test_tables():
    d = AE.DECODE_CASES
    assert len(set(d)) == len(d) and len(set(AE.PREFILL_CASES)) == len(AE.PREFILL_CASES)
    for hd in (64, 128):
        for ctx in (160, 1024):
            assert {c.G for c in d if c.hd == hd and c.ctx == ctx and c.B == 1 and c.KVH == 2} == set(range(1, 9))
        assert {c.B for c in d if c.hd == hd and c.G == AE.BATCH_G[hd]} == {1, 2, 3, 4, 8}
        for ctx, chunk in AE.GROWN.items():
            assert AE.DCase(1, 2 * AE.GROWN_G[hd], 2, hd, ctx) in d and AE.Plan(hd, ctx).c == chunk
    assert AE.Plan(128, 8192).chunks == 64
    p = AE.PREFILL_CASES
    for hd in (64, 128):
        for G in (1, 4, 8):
            got = {(B, S, start) for B, H, KVH, h, S, start, ctx in p if h == hd and H // KVH == G}
            assert got >= set(AE.PREFILL_SHAPES)
    assert {S for B, H, KVH, hd, S, start, ctx in p if start == 0} == {1, 17, 65, 129}
    tight = sum(ctx == start + S for B, H, KVH, hd, S, start, ctx in p)
    assert abs(2 * tight - len(p)) <= 2
    assert any(S > 128 and start >= 64 for B, H, KVH, hd, S, start, ctx in p)


# ---- decode ----------------------------------------------------------------------------

def test_d1_levels(dec):
    q, k, v = dec["q"], dec["k"], dec["v"]
    case = dec["case"]
    assert bool(((k == 0) | (k == AE.KOFF)).all()) and bool((v.abs() >= 1).all()) and bool((v.abs() <= 2).all())
    assert bool(((q != 0).sum(-1) == 1).all()) and bool(((q == 0) | (q == AE.QVAL)).all())
    assert torch.equal(v.to(AE.I64), dec["vint"])
    for b in range(case.B):  # heads of one kv head use different columns
        for kh in range(case.KVH):
            assert dec["cols"][b, kh * case.G:(kh + 1) * case.G].unique().numel() == case.G
    kvh = torch.arange(case.H) // case.G
    scores = torch.einsum("bhd,bhkd->bhk", q.to(F64), k.to(F64)[:, kvh]) * dec["scale"]
    AE.check_levels(scores, dec["sel"])


def test_d2_rounding(dec):
    case = dec["case"]
    lo, hi, dist = 10 ** 9, 0, 1.0
    for p in _all_positions(case):
        n, S, _ = AE.decode_ref(dec, p)
        a, b, d = AE.check_rounding(n, S)
        lo, hi, dist = min(lo, a), max(hi, b), min(dist, d)
    print(f"{AE.decode_id(case)}: counts {lo} .. {hi}, smallest midpoint distance {dist:.3g}")


def test_d3_visibility(dec):
    case = dec["case"]
    pairs = 0
    for p in AE.decode_positions(case.plan):
        n, S, _ = AE.decode_ref(dec, p)
        for b in range(case.B):
            for kh in range(case.KVH):
                hs = slice(kh * case.G, (kh + 1) * case.G)
                pairs += AE.check_visibility(dec["sel"][b, hs, :p + 1], n[b, hs], S[b, hs], dec["vint"][b, kh, :p + 1])
    print(f"{AE.decode_id(case)}: {pairs} (row, counted key) pairs, none blind")


def test_d_rescale_and_coverage(dec):
    """At pos = ctx - 1 every head has counted keys in every unit of the split
    that is not dark, and meets dark units where decode_dark puts them."""
    case = dec["case"]
    plan = case.plan
    AE.decode_coverage(dec)
    r = AE.decode_rescale(dec, case.ctx - 1)
    x0 = (torch.arange(case.H) // case.G) % 2 == 0
    for name, (before, after) in r.items():
        print(name, "before", before.all().item(), "after", after.all().item())
    if plan.trips >= 2:
        assert bool(r["trip"][0].all()) and bool(r["trip"][1].all())
    else:
        assert plan.hd == 64 and plan.c == 128
    assert bool(r["group"][0].all()) and bool(r["group"][1].all())
    assert bool(r["wave"][1].all())
    assert plan.chunks >= 2
    assert plan.chunks == 2 or plan.chunks >= 5
    if plan.chunks >= 5:
        assert bool(r["wave"][0].all()) and bool(r["chunk"][1].all())
    else:
        assert bool(r["chunk"][1][:, x0].all())
    assert not bool(r["chunk"][0].any())  # key 0 is in chunk 0


def test_d_emulation_exact(dec):
    case = dec["case"]
    for p in [-1] + _all_positions(case):
        k, v = AE.tempt(dec["k"], dec["v"], max(0, p + 1))
        got = AE.emulate_decode(dec["q"], k, v, p, dec["scale"])
        assert torch.equal(got, AE.decode_ref(dec, p)[2]), p
    assert not bool(AE.decode_ref(dec, -1)[2].any())


def _cannot_show(case, mistake):
    if mistake.get("wrong_gqa"):
        return case.G == 1
    if mistake.get("unscaled", ("", ""))[1] == "trip":
        return case.plan.trips < 2
    return False


@pytest.mark.parametrize("mistake", AE.MISTAKES, ids=AE.mistake_id)
def test_d_mistake(dec, mistake):
    case = dec["case"]
    hits = 0
    right = torch.arange(case.H) // case.G
    for p in AE.mistake_positions(case):
        k, v = AE.tempt(dec["k"], dec["v"], p + 1)
        want = AE.decode_ref(dec, p)[2]
        info = {}
        got = AE.emulate_decode(dec["q"], k, v, p, dec["scale"], info=info, **mistake)
        if not info["hit"]:
            assert torch.equal(got, want), p
            continue
        hits += 1
        assert not torch.equal(got, want), p
        if mistake.get("wrong_gqa"):  # every head that reads another kv head
            moved = (torch.arange(case.H) % case.KVH) != right
            assert bool((got != want).any(-1)[:, moved].all()), p
    assert (hits == 0) == _cannot_show(case, mistake), hits


# ---- prefill ---------------------------------------------------------------------------

def _groups(case):
    B, H, KVH, hd, S, start, ctx = case
    G = H // KVH
    return [(b, kh, slice(kh * G, (kh + 1) * G)) for b in range(B) for kh in range(KVH)]


def test_p1_levels(pre):
    case = pre["case"]
    B, H, KVH, hd, S, start, ctx = case
    nk = start + S
    q, k, v = pre["q"], pre["k"], pre["v"]
    assert bool(((k == 0) | (k == AE.KOFF)).all()) and bool(((q == 0) | (q == AE.QVAL)).all())
    assert bool(((q != 0).sum(-1) == 1).all())
    assert bool((k[:, :, nk:] == 0).all()) and bool((v[:, :, nk:] == AE.TEMPT_V).all())
    assert torch.equal(v[:, :, :nk].to(AE.I64), pre["vint"]) and bool((pre["vint"].abs() <= 2).all())
    for b, kh, hs in _groups(case):
        scores = torch.einsum("shd,kd->hsk", q[b, :, hs].float(), k[b, kh, :nk].float()).to(F64) * pre["scale"]
        chosen = pre["selk"][b, kh].t()[pre["cols"][b, :, hs].t()]  # by the row's column, whatever the mask
        AE.check_levels(scores, chosen)


def test_p2_rounding(pre):
    n, S, _ = AE.prefill_ref(pre)
    lo, hi, dist = AE.check_rounding(n, S)
    print(f"{AE.prefill_id(pre['case'])}: counts {lo} .. {hi}, smallest midpoint distance {dist:.3g}")


def test_p3_visibility(pre):
    case = pre["case"]
    n, S, _ = AE.prefill_ref(pre)
    pairs = 0
    for b, kh, hs in _groups(case):
        sel = AE.prefill_sel(pre, b, kh)
        rows = sel.shape[0] * sel.shape[1]
        pairs += AE.check_visibility(sel.reshape(rows, -1), n[b, :, hs].t().reshape(rows),
                                     S[b, :, hs].transpose(0, 1).reshape(rows, -1), pre["vint"][b, kh])
    print(f"{AE.prefill_id(case)}: {pairs} (row, counted key) pairs, none blind")


def test_p_dark_tile(pre):
    """Beyond 128 keys, one key tile is deselected whole: rows that reach
    past it keep m = 0 through a tile of probabilities that are all 0."""
    case = pre["case"]
    B, H, KVH, hd, S, start, ctx = case
    for kh in range(KVH):
        t = AE.prefill_dark_tile(case, kh)
        if t is None:
            assert start + S <= 128
            continue
        assert not bool(pre["selk"][:, kh, 64 * t:64 * t + 64].any())
        assert start + S - 1 >= 64 * t + 64  # the last row sees all of it, after key 0


def test_p_emulation_exact(pre):
    B, H, KVH, hd, S, start, ctx = pre["case"]
    got = PR.emulate(pre["q"], pre["k"], pre["v"], start, pre["scale"])
    assert torch.equal(got, AE.prefill_ref(pre)[2])


@pytest.mark.parametrize("mistake", [dict(mask_shift=1), dict(mask_shift=-1), dict(wrong_gqa=True)],
                         ids=AE.mistake_id)
def test_p_mistake(pre, mistake):
    case = pre["case"]
    B, H, KVH, hd, S, start, ctx = case
    G = H // KVH
    want = AE.prefill_ref(pre)[2]
    got = PR.emulate(pre["q"], pre["k"], pre["v"], start, pre["scale"], **mistake)
    changed = (got != want).any(-1)  # [B, S, H]
    kvh = torch.arange(H) // G
    own = torch.arange(S) + start
    if mistake.get("wrong_gqa"):
        moved = (torch.arange(H) % KVH) != kvh
        assert bool(moved.any()) == (G > 1)
        assert bool(changed[:, :, moved].all()) and not bool(changed[:, :, ~moved].any())
    elif mistake["mask_shift"] == -1:  # the row loses its own key: a counted key wherever its column selects it
        lost = pre["selk"][:, kvh][:, :, own].gather(3, pre["cols"].permute(0, 2, 1)[..., None])[..., 0]  # [B, H, S]
        assert bool(lost.any())
        assert torch.equal(changed, lost.permute(0, 2, 1))
    else:  # the row gains key start + s + 1, where the cache has one; a row beyond the prompt is selected always
        nxt = own + 1
        has = nxt < ctx
        k0 = pre["k"][:, kvh][:, :, nxt.clamp(max=ctx - 1)]  # [B, H, S, hd]
        gained = (k0.gather(3, pre["cols"].permute(0, 2, 1)[..., None])[..., 0] == 0) & has
        assert bool(has.any()) == (S > 1 or ctx > start + S)
        assert not bool((changed.permute(0, 2, 1) & ~gained).any())
        assert bool(changed.any()) == bool(gained.any()) and bool(gained.any()) == bool(has.any())
