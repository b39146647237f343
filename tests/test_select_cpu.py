"""Token selection (vgpu.ops.select) without a GPU: every refusal fires before
the library loads, the fp64 reference of tests/_select_ref.py agrees with
torch.topk + softmax + cumsum, and the case table has the power to notice a
wrong kernel: an emulation of the kernels' chunked route passes every case and
every mutant of the definition fails at least one."""
import numpy as np
import pytest
import torch

import _select_ref as R
from vgpu.ops import select as S

BF = torch.bfloat16
I64 = torch.int64


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the kernel library was loaded")
    monkeypatch.setattr(S, "load_kernels", boom)


def _args(B=2, V=16, T=3, **over):
    a = dict(logits=torch.zeros(B, V, dtype=BF), ws=torch.zeros(1024, dtype=torch.int32),
             step=torch.zeros(1, dtype=I64), pos=torch.zeros(1, dtype=I64), next_tok=torch.zeros(B, 1, dtype=I64),
             out=torch.zeros(B, T, dtype=I64))
    a.update(over)
    return a


def _sample_args(B=2, V=16, T=3, **over):
    a = _args(B, V, T)
    a.update(u=torch.zeros(T, B), temperature=1.0, top_k=4, top_p=0.9)
    a.update(over)
    return a


GREEDY_REFUSALS = [
    (dict(logits=torch.zeros(16, dtype=BF)), r"logits: shape \(16,\), expected \[B, V\]"),
    (dict(logits=torch.zeros(5, 16, dtype=BF)), "batch 5 not in"),
    (dict(logits=torch.zeros(2, 12, dtype=BF)), "vocab 12 not a multiple of 8"),
    (dict(logits=torch.zeros(2, 0, dtype=BF)), "vocab 0 not a multiple of 8"),
    (dict(out=torch.zeros(2, 0, dtype=I64)), "out: shape .* T >= 1"),
    (dict(out=torch.zeros(3, 3, dtype=I64)), "out: shape"),
    (dict(out=torch.zeros(6, dtype=I64)), "out: shape"),
    (dict(eos=16), "eos: 16"),
    (dict(eos=-2), "eos: -2"),
    (dict(logits=torch.zeros(2, 32, dtype=BF)[:, ::2]), "logits: not contiguous"),
    (dict(logits=torch.zeros(2, 16)), "logits: dtype torch.float32"),
    (dict(step=torch.zeros(2, dtype=I64)), r"step: shape \(2,\)"),
    (dict(step=torch.zeros(1, dtype=torch.int32)), "step: dtype torch.int32"),
    (dict(pos=torch.zeros(1, 1, dtype=I64)), r"pos: shape \(1, 1\)"),
    (dict(pos=torch.zeros(1)), "pos: dtype torch.float32"),
    (dict(next_tok=torch.zeros(2, dtype=I64)), r"next_tok: shape \(2,\)"),
    (dict(next_tok=torch.zeros(2, 1, dtype=torch.int32)), "next_tok: dtype"),
    (dict(out=torch.zeros(2, 6, dtype=I64)[:, ::2]), "out: not contiguous"),
    (dict(out=torch.zeros(2, 3, dtype=torch.int32)), "out: dtype"),
    (dict(ws=torch.zeros(4, 4, dtype=torch.int32)), "ws: shape"),
    (dict(ws=torch.zeros(16, dtype=I64)), "ws: dtype"),
    (dict(), "logits: on cpu, expected a GPU tensor"),  # everything else in order: the device comes last
]

SAMPLE_REFUSALS = [
    (dict(temperature=0.0), "temperature 0.0"),
    (dict(temperature=-1.0), "temperature -1.0"),
    (dict(temperature=float("nan")), "temperature nan"),
    (dict(temperature=float("inf")), "temperature inf"),
    (dict(top_k=0), "top_k 0"),
    (dict(top_k=65), "top_k 65"),
    (dict(top_k=2.0), "top_k 2.0"),
    (dict(top_p=0.0), "top_p 0.0"),
    (dict(top_p=1.5), "top_p 1.5"),
    (dict(top_p=float("nan")), "top_p nan"),
    (dict(u=torch.zeros(2, 3)), r"u: shape \(2, 3\), expected \(3, 2\)"),
    (dict(u=torch.zeros(3)), r"u: shape \(3,\)"),
    (dict(u=torch.zeros(3, 2, dtype=torch.float64)), "u: dtype torch.float64"),
    (dict(u=torch.zeros(2, 3).t()), "u: not contiguous"),
    (dict(logits=torch.zeros(5, 16, dtype=BF)), "batch 5 not in"),
    (dict(out=torch.zeros(2, 0, dtype=I64)), "out: shape .* T >= 1"),
    (dict(), "logits: on cpu, expected a GPU tensor"),
]


@pytest.mark.parametrize("over, msg", GREEDY_REFUSALS, ids=[m for _, m in GREEDY_REFUSALS])
def test_greedy_refuses_before_loading(no_library, over, msg):
    with pytest.raises(ValueError, match=msg):
        S.greedy(**_args(**over))


@pytest.mark.parametrize("over, msg", SAMPLE_REFUSALS, ids=[m for _, m in SAMPLE_REFUSALS])
def test_sample_refuses_before_loading(no_library, over, msg):
    with pytest.raises(ValueError, match=msg):
        S.sample(**_sample_args(**over))


def test_shape_reason_and_workspace_refuse_before_loading(no_library):
    assert S.shape_reason(1, 128256, 64) is None and S.shape_reason(8, 8) is None
    assert "batch 6" in S.shape_reason(6, 16)
    assert "vocab 20" in S.shape_reason(1, 20)
    assert "top_k 65" in S.shape_reason(1, 16, 65) and "top_k 0" in S.shape_reason(1, 16, 0)
    assert S.params_reason(0.7, 50, 0.9) is None and S.params_reason(1e-3, 1, 1.0) is None
    for call in (lambda: S.workspace_bytes(5, 16), lambda: S.workspace_bytes(1, 4), lambda: S.chunk(12)):
        with pytest.raises(ValueError, match="select shape not supported"):
            call()
    assert S.MAX_TOP_K == 64


def test_generate_refuses_before_any_gpu_work(no_library):
    """generate_native's own refusals need neither the library nor a GPU."""
    from vgpu.models.llama import Llama, LlamaConfig
    m = Llama(LlamaConfig.tiny())
    kv = m.new_kv_cache(1, 16)
    toks = torch.zeros(1, 5, dtype=I64)
    for kw, msg in [(dict(max_new=0), "max_new"), (dict(max_new=13), "exceeds"), (dict(max_new=12, start=1), "exceeds"),
                    (dict(max_new=4, temperature=1.0, top_k=65), "top_k 65"),
                    (dict(max_new=4, temperature=-1.0), "temperature"),
                    (dict(max_new=4, temperature=1.0, top_k=4, top_p=0.0), "top_p"), (dict(max_new=4, eos=512), "eos")]:
        with pytest.raises(ValueError, match=msg):
            m.generate_native(toks, kv, **kw)


# ---- the reference against stock torch, on rows without ties ------------------------------

def test_reference_agrees_with_topk_softmax_cumsum():
    g = torch.Generator().manual_seed(5)
    V = 4096
    for trial in range(40):
        row = torch.unique(torch.randn(V, generator=g).mul(4).to(BF))  # distinct bf16 values, so no ties
        row = row[torch.randperm(row.numel(), generator=g)]
        x = row.double()
        k = int(torch.randint(1, 65, (1,), generator=g))
        T = R.f32(0.25 + 2 * torch.rand(1, generator=g).item())
        top_p = R.f32(0.05 + 0.95 * torch.rand(1, generator=g).item())
        u = R.f32(torch.rand(1, generator=g).item())
        val, idx = torch.topk(x, k)
        assert np.array_equal(R.ordering(x.numpy(), k), idx.numpy())
        cum = torch.softmax(val / T, 0).cumsum(0)  # W_k = 1
        m = int((cum >= top_p).nonzero()[0]) + 1 if (cum >= top_p).any() else k
        j = (cum[:m] > u * cum[m - 1]).nonzero()
        j = int(j[0]) if j.numel() else m - 1
        if min(abs(cum - top_p).min().item(), abs(cum[:m] - u * cum[m - 1]).min().item()) < 1e-9:
            continue  # the two fp64 routes round differently: not a draw either decides
        assert R.choose_ref(x.numpy(), R.ordering(x.numpy(), k), T, top_p, u) == (int(idx[j]), m, j), trial


def test_first_index_is_the_ordering():
    for c in R.cases():
        if c["greedy"] and c["logits"].shape[1] <= 3 * R.CHUNK + 8:
            want = [int(R.ordering(r, 1)[0]) for r in c["logits"].double().numpy()]
            assert R.first_index(c["logits"]).tolist() == want, c["name"]


# ---- the table's power ------------------------------------------------------------------

def test_table_covers_what_the_issue_lists():
    tab = R.cases()
    greedy = [c for c in tab if c["greedy"] and c["name"].startswith("greedy")]
    assert {c["logits"].shape[1] for c in greedy} == set(R.greedy_vocabs())
    for V in R.greedy_vocabs():
        assert {c["logits"].shape[0] for c in greedy if c["logits"].shape[1] == V} >= ({1, 2, 3, 4} if V < 99 else
                                                                                         set(R.BATCHES))
        firsts = {int(t) for c in greedy if c["logits"].shape[1] == V for t in R.expected(c)["out"][:, 0]}
        edges = range(R.CHUNK, V, R.CHUNK)
        assert firsts >= {0, 7, 8 % V, V - 1} | {e - 1 for e in edges} | set(edges), V
    assert {c["top_k"] for c in tab if c["name"].startswith("uniform")} == {1, 2, 8, 64}
    assert {c["temperature"] for c in tab if c["name"].startswith("graded")} == {0.5, 1.0, 2.0}
    assert any(c["logits"].shape[1] == R.VOCAB and not c["greedy"] for c in tab)


def test_every_nucleus_member_is_drawn_and_by_a_wide_margin():
    """Per sampling case: the u values reach every member of the nucleus (for
    the midpoint cases, one u each), and in the graded cases top_p and every
    u sit at least 2^-10 (relative) from the nearest cumulative mass, 64 times
    the 2^-16 that fp32 can move them by."""
    for c in R.cases():
        if c["greedy"] or not c["name"].startswith(("uniform", "graded")):
            continue
        x = c["logits"].double().numpy()
        for b in range(x.shape[0]):
            cand = R.ordering(x[b], c["top_k"])
            hits = [R.choose_ref(x[b], cand, c["temperature"], c["top_p"], float(u))[1:] for u in c["u"][:, b]]
            m = hits[0][0]
            assert {j for _, j in hits} == set(range(m)), c["name"]
            if not c["name"].endswith(" u"):
                assert len(hits) == m, c["name"]
            if c["name"].startswith("graded"):
                w = np.exp((x[b][cand] - x[b][cand[0]]) / c["temperature"])
                cum = np.cumsum(w)
                assert (w[:m] / cum[m - 1]).min() >= 2.0 ** -8, c["name"]
                assert c["top_p"] == 1.0 or np.abs(cum / cum[-1] - c["top_p"]).min() >= 2.0 ** -10, c["name"]
                for u in c["u"][:, b]:
                    assert np.abs(cum[:m] / cum[m - 1] - float(u)).min() >= 2.0 ** -10, c["name"]


def test_emulation_of_the_chunked_route_passes_every_case():
    for c in R.cases():
        assert R.same(R.simulate(c, emulate=True), R.expected(c)), c["name"]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_fails_a_case(mutant):
    assert any(not R.same(R.simulate(c, mut=(mutant,)), R.expected(c)) for c in R.cases()), mutant


def test_order_keys_realise_the_ordering():
    """All 65 536 bf16 patterns: sorting by the kernels' 16-bit key is the ordering."""
    bits = np.arange(65536, dtype=np.uint16)
    x = torch.from_numpy(bits.view(np.int16).copy()).view(BF).double().numpy()
    key = R.order_keys(bits)
    by_key = np.lexsort((np.arange(65536), -key))
    # NaNs all share key 0, and +0 / -0 one key: the index decides among them in both
    assert np.array_equal(by_key, R.ordering(x, 65536))
    ok = key > 0
    assert np.array_equal(R.key_values(key[ok]).astype(np.float64) + 0.0, x[ok] + 0.0)
