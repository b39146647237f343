"""Token selection on the device (native/kernels/select.hip through
vgpu.ops.select) against the case table and fp64 reference of
tests/_select_ref.py, exactly: greedy, sampling (cases built so that fp32 and
fp64 cannot disagree), the advance of step / pos / next_tok / out; then
Llama.generate_native and LlamaFp8.generate_native end to end against host
loops over prefill_native / decode_native."""
import pytest
import torch

import _decode_ref as D
import _select_ref as R
from vgpu.models.llama import LlamaFp8
from vgpu.ops import select as S

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
I64 = torch.int64
PAD = 4            # guard words around every buffer the kernels write
FENCE = -123456789


def run_gpu(c):
    """The case's calls on the GPU.  out, next_tok, step and pos are slices of
    one fenced int64 buffer; returns the state and that buffer before / after."""
    logits = c["logits"].cuda()
    B, V = logits.shape
    T = c["T"]
    n = [1, 1, B, B * T]  # step, pos, next_tok, out
    raw = torch.full((PAD + sum(x + PAD for x in n),), FENCE, dtype=I64, device="cuda")
    at, views = PAD, []
    for x in n:
        views.append(raw[at:at + x])
        at += x + PAD
    step, pos, nxt, out = views[0], views[1], views[2].view(B, 1), views[3].view(B, T)
    step.fill_(c["s0"])
    pos.fill_(c["pos0"])
    nxt.fill_(R.GUARD)
    out.copy_(c["out0"])
    before = raw.clone()
    ws = torch.empty(S.workspace_bytes(B, V) // 4, dtype=torch.int32, device="cuda")
    u = None if c["greedy"] else c["u"].cuda()
    for _ in range(c["calls"]):
        if c["greedy"]:
            S.greedy(logits, ws, step, pos, nxt, out, c["eos"])
        else:
            S.sample(logits, ws, step, pos, nxt, out, u, c["temperature"], c["top_k"], c["top_p"], c["eos"])
    after = raw.cpu()
    fences = torch.ones(raw.numel(), dtype=torch.bool)
    at = PAD
    for x in n:
        fences[at:at + x] = False
        at += x + PAD
    assert bool((after[fences] == FENCE).all()), f"{c['name']}: a guard word was written"
    return dict(out=out.cpu(), next_tok=nxt.cpu(), step=int(step.item()), pos=int(pos.item())), before.cpu(), after


def _check_group(prefixes):
    picked = [c for c in R.cases() if c["name"].startswith(prefixes)]
    assert picked
    bad = []
    for c in picked:
        got, _, _ = run_gpu(c)
        want = R.expected(c)
        if not R.same(got, want):
            bad.append((c["name"], got["out"].tolist(), want["out"].tolist(), got["step"], got["pos"]))
    assert not bad, f"{len(bad)} of {len(picked)} cases differ; first: {bad[0]}"


def test_chunk_and_workspace(gpu_build):
    for V in R.greedy_vocabs():
        assert S.chunk(V) == R.CHUNK  # the table's edges are the kernels' edges
    for B in R.BATCHES:
        chunks = -(-R.VOCAB // R.CHUNK)
        assert S.workspace_bytes(B, R.VOCAB) == B * chunks * S.MAX_TOP_K * 8
    lib = S._lib()
    assert lib.vgpu_select_supported(1, R.VOCAB, 64) == 1
    for B, V, k in [(5, 16, 1), (1, 12, 1), (1, 0, 1), (1, 16, 0), (1, 16, 65)]:
        assert lib.vgpu_select_supported(B, V, k) == 0


def test_greedy_exact(gpu_build):
    _check_group("greedy")


def test_top_k_1_is_greedy(gpu_build):
    _check_group("top1")


def test_sampling_uniform_exact(gpu_build):
    _check_group("uniform")


def test_sampling_graded_exact(gpu_build):
    _check_group("graded")


def test_sampling_non_finite(gpu_build):
    _check_group("sample non-finite")


def test_advance_and_eos(gpu_build):
    _check_group(("advance", "eos"))
    for c in R.cases():
        if c["name"].startswith("advance s ="):  # outside [0, T): unchanged to the byte
            _, before, after = run_gpu(c)
            assert torch.equal(before, after), c["name"]


def test_small_workspace_is_refused(gpu_build):
    c = R.cases()[0]
    B, V = c["logits"].shape
    z = torch.zeros(1, dtype=I64, device="cuda")
    with pytest.raises(ValueError, match="ws: 8 bytes, needs"):
        S.greedy(c["logits"].cuda(), torch.zeros(2, dtype=torch.int32, device="cuda"), z, z.clone(),
                 torch.zeros(B, 1, dtype=I64, device="cuda"), torch.zeros(B, 1, dtype=I64, device="cuda"))


# ---- end to end -------------------------------------------------------------------------

PROMPT, NEW = 5, 12


def _prompt(ci, B):
    g = torch.Generator().manual_seed(31 + 10 * ci + B)
    return torch.randint(0, D.CONFIGS[ci].vocab, (B, PROMPT), generator=g).cuda()


def _host_greedy(m, toks, kv):
    """prefill_native / decode_native with the CPU ordering applied to the returned logits."""
    B = toks.shape[0]
    pos = torch.zeros(1, dtype=I64, device="cuda")
    logits = m.prefill_native(toks, kv, 0)
    out = []
    for i in range(NEW):
        t = torch.from_numpy(R.first_index(logits.view(B, -1).cpu()))
        out.append(t)
        if i < NEW - 1:
            pos.fill_(PROMPT + i)
            logits = m.decode_native(t.view(B, 1).cuda(), kv, pos)
    return torch.stack(out, 1)


def _same_caches(a, b):
    return all(torch.equal(ka, kb) and torch.equal(va, vb) for (ka, va), (kb, vb) in zip(a, b))


def _greedy_equalities(m, ci, B):
    toks = _prompt(ci, B)
    kv_host, kv_plain, kv_graph = (D.new_cache(m, B, D.CTX, BF, "cuda") for _ in range(3))
    want = _host_greedy(m, toks, kv_host)
    plain = m.generate_native(toks, kv_plain, NEW, graph=False)
    assert plain.dtype == I64 and tuple(plain.shape) == (B, NEW)
    assert torch.equal(plain.cpu(), want)
    assert _same_caches(kv_plain, kv_host)
    graph = m.generate_native(toks, kv_graph, NEW, graph=True)
    assert torch.equal(graph, plain)
    assert _same_caches(kv_graph, kv_plain)
    return toks, plain


@pytest.mark.parametrize("ci", [0, 1])
@pytest.mark.parametrize("B", [1, 2])
def test_generate_greedy(gpu_build, ci, B):
    m = D.model_as(ci, BF, "cuda")
    toks, plain = _greedy_equalities(m, ci, B)
    # eos: the token row 0 emits at step 3; from its first appearance on, a row holds eos
    eos = int(plain[0, 3])
    got = m.generate_native(toks, D.new_cache(m, B, D.CTX, BF, "cuda"), NEW, eos=eos).cpu()
    assert bool((got[0, 4:] == eos).all())
    for b in range(B):
        hit = (plain[b].cpu() == eos).nonzero()
        n = int(hit[0]) + 1 if hit.numel() else NEW
        assert torch.equal(got[b, :n], plain[b, :n].cpu()) and bool((got[b, n:] == eos).all())


@pytest.mark.parametrize("ci", [0, 1])
@pytest.mark.parametrize("B", [1, 2])
def test_generate_sampled(gpu_build, ci, B):
    m = D.model_as(ci, BF, "cuda")
    toks = _prompt(ci, B)
    kw = dict(temperature=1.0, top_k=8, top_p=0.9, seed=3)
    kv_host, kv_plain, kv_graph = (D.new_cache(m, B, D.CTX, BF, "cuda") for _ in range(3))
    # the host loop: vgpu.ops.select.sample step by step
    V = m.cfg.vocab
    u = torch.rand(NEW, B, generator=torch.Generator().manual_seed(3)).cuda()
    out = torch.zeros(B, NEW, dtype=I64, device="cuda")
    nxt = torch.zeros(B, 1, dtype=I64, device="cuda")
    step = torch.zeros(1, dtype=I64, device="cuda")
    pos = torch.full((1,), PROMPT - 1, dtype=I64, device="cuda")
    ws = torch.empty(S.workspace_bytes(B, V) // 4, dtype=torch.int32, device="cuda")
    logits = m.prefill_native(toks, kv_host, 0)
    for i in range(NEW):
        S.sample(logits.view(B, V), ws, step, pos, nxt, out, u, 1.0, 8, 0.9)
        assert int(step) == i + 1 and int(pos) == PROMPT + i
        if i < NEW - 1:
            logits = m.decode_native(nxt, kv_host, pos)
    plain = m.generate_native(toks, kv_plain, NEW, graph=False, **kw)
    assert torch.equal(plain, out) and _same_caches(kv_plain, kv_host)
    graph = m.generate_native(toks, kv_graph, NEW, graph=True, **kw)
    assert torch.equal(graph, plain) and _same_caches(kv_graph, kv_plain)


def test_generate_fp8(gpu_build):
    m = LlamaFp8.from_llama(D.model_as(0, BF, "cuda"))
    for B in (1, 2):
        _greedy_equalities(m, 0, B)


def test_generate_refusals(gpu_build):
    m = D.model_as(0, BF, "cuda")
    toks = _prompt(0, 1)
    short = D.new_cache(m, 1, PROMPT + NEW - 2, BF, "cuda")  # one row too few
    with pytest.raises(ValueError, match="exceeds"):
        m.generate_native(toks, short, NEW)
    exact = D.new_cache(m, 1, PROMPT + NEW - 1, BF, "cuda")
    assert tuple(m.generate_native(toks, exact, NEW).shape) == (1, NEW)
    kv = D.new_cache(m, 1, D.CTX, BF, "cuda")
    with pytest.raises(ValueError, match="max_new"):
        m.generate_native(toks, kv, 0)
    with pytest.raises(ValueError, match="top_k 65"):
        m.generate_native(toks, kv, 4, temperature=1.0, top_k=65)
