"""ops.lm_score_ (lm_score.hip) against fp64 on the same bf16 residual, the same bf16 or decoded-FP8 LM head and the
same scales, and the engine's prompt scoring on top of it (docs/PROMPT_LOGPROBS.md).

The bounds are derived, with u = 2^-24 (fp32 unit roundoff):
  logit    z = ((x . W'[v]) * scale[v]) * inv:  (dim + 8) u sum_k |x_k W'_vk| |scale| inv for the fp32 accumulation of
           dim exact bf16 products in whatever order the MFMA takes, plus |z| ((dim + 8) / 2 + 4 + 2) u: the row's sum
           of squares is dim positive terms (relative (dim + 8) u, halved by the square root), the division, eps and
           rsqrtf are 4 u, the two multiplications 2 u.
  z_top    the largest logit bound of the row (max is 1-Lipschitz).
  lse      the same (log-sum-exp is 1-Lipschitz), plus the sum's relative error u (sum_v p_v |z_v - max| + 64): every
           exp argument is a chain of differences whose roundings add up to u |z_v - max|, and one term passes at
           most 8 expf (2 u each), 8 products and 18 additions on its way through lane, row, wave, slab and merge;
           plus logf's 2 u |log S| and the last addition's u |lse|.
"""
import math

import pytest
import torch

from p2p_llm_tunnel_amd import ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 1e-5
SHAPES = [(560, 64, 1), (560, 256, 17), (4112, 1024, 64)]
TIE = (100, -3)  # the planted tie's columns: W'[V - 3] = W'[100], in different slabs


def reference(x, w, scale, eps, dim):
    """fp64 (z, per-logit bound) of bf16 rows ``x`` against decoded weights ``w`` (fp32 or bf16 values) and fp32 row
    scales (None: 1)."""
    xd, wd = x.double(), w.double()
    sc = scale.double() if scale is not None else torch.ones(w.shape[0], dtype=torch.float64)
    inv = 1.0 / torch.sqrt((xd * xd).mean(1) + eps)
    z = (xd @ wd.T) * sc[None, :] * inv[:, None]
    mag = (xd.abs() @ wd.abs().T) * sc.abs()[None, :] * inv[:, None]
    return z, (dim + 8) * U * mag + z.abs() * ((dim + 8) / 2 + 6) * U


def lse_bound(z, bz):
    m = z.max(1).values
    lse = torch.logsumexp(z, 1)
    p = torch.exp(z - lse[:, None])
    rel = U * ((p * (z - m[:, None]).abs()).sum(1) + 64)
    return lse, bz.max(1).values + rel + 2 * U * (lse - m).abs() + U * lse.abs()


def make_case(V, dim, rows, fp8, seed=0):
    """Host tensors of one case. Row ``rows - 1`` has the planted tie for its maximum; row 5 (when there is one) is
    off; the targets cycle through column 0, column V - 1 and both sides of the first slab boundary."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, dim, generator=g) * 1.5).bfloat16()
    w = torch.randn(V, dim, generator=g) * (4.0 / math.sqrt(dim))
    x[rows - 1] = (w[TIE[0]] * 3 + torch.randn(dim, generator=g) * 0.05).bfloat16()
    w[TIE[1]] = w[TIE[0]]
    slab = ops.lm_score_plan(V, dim, rows).slab
    cycle = [0, V - 1, slab, slab - 1, V // 2]
    target = torch.tensor([cycle[m % len(cycle)] for m in range(rows)], dtype=torch.int32)
    if rows > 5:
        target[5] = -1
    if fp8:
        q, scale = ops.quantize_weight_fp8(w)
        return x, q, scale, q.float(), target
    return x, w.bfloat16(), None, w.bfloat16().float(), target


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("V,dim,rows", SHAPES)
def test_lm_score_against_fp64(V, dim, rows, fp8):
    x, head, scale, decoded, target = make_case(V, dim, rows, fp8)
    z, bz = reference(x, decoded, scale, EPS, dim)
    lse, b_lse = lse_bound(z, bz)
    top2 = z.topk(2, 1)
    # Rows whose fp64 argmax the bound cannot promise: the planted tie, and at most one more (the seed's doing).
    clear = (top2.values[:, 0] - top2.values[:, 1]) > 2 * bz.max(1).values
    assert not clear[rows - 1] and int((~clear).sum()) <= 2

    dev = torch.device("cuda:0")
    out = [torch.full((rows,), 123.0, device=dev) for _ in range(3)] + \
          [torch.full((rows,), -7, dtype=torch.int32, device=dev)]
    ops.lm_score_(x.to(dev), head.to(dev), None if scale is None else scale.to(dev), EPS, target.to(dev), *out)
    got_lse, got_zt, got_top, got_id = (t.cpu() for t in out)

    on = target >= 0
    for t, sentinel in zip((got_lse, got_zt, got_top, got_id), (123.0, 123.0, 123.0, -7)):
        assert bool((t[~on] == sentinel).all()), "a row that is off had an output written"
    rws = torch.arange(rows)[on]
    tg = target[on].long()
    ratios = {"lse": ((got_lse[on].double() - lse[on]).abs() / b_lse[on]).max().item(),
              "z_target": ((got_zt[on].double() - z[rws, tg]).abs() / bz[rws, tg]).max().item(),
              "z_top": ((got_top[on].double() - top2.values[on, 0]).abs() / bz.max(1).values[on]).max().item()}
    print(f"lm_score V={V} dim={dim} rows={rows} {'fp8' if fp8 else 'bf16'}: largest error / bound {ratios}")
    assert max(ratios.values()) <= 1.0
    check = on & clear
    assert torch.equal(got_id[check].long(), top2.indices[check, 0])
    assert int(got_id[rows - 1]) == TIE[0]  # the tie: both columns are the row's maximum, the lower id wins


@pytest.mark.parametrize("weight_dtype", ["bf16", "fp8"])
def test_engine_scores_prompt(weight_dtype):
    from p2p_llm_tunnel_amd.models.engine import Engine, Request

    def run(eng, reqs):
        for r in reqs:
            eng.submit(r)
        toks = []
        for r in reqs:
            toks.append(list(iter(r.out.get, None)))
        return toks

    g = torch.Generator().manual_seed(1)
    prompt, p1, p2 = (torch.randint(0, 256, (n,), generator=g).tolist() for n in (40, 30, 90))
    eng = Engine(config="tiny", max_batch=4, prefix_cache=True, prompt_logprobs=True, weight_dtype=weight_dtype)
    try:
        alone = Request(prompt, 0, score=True)
        assert run(eng, [alone]) == [[]]
        # The step that ran the prompt's 40 rows, alone, left them in resid: the reference's input.
        dec = eng.model.fused_decoder()
        torch.cuda.synchronize()
        x = dec.workspace_views()["resid"][:len(prompt)].cpu()
        head = dec.weights[dec.table.index("lm_head")].cpu()
        scale = dec.weights[dec.table.scale_index("lm_head")].cpu() if weight_dtype == "fp8" else None
        batched = Request(prompt, 0, score=True)
        gen = run(eng, [Request(p1, 6), Request(p2, 6), batched])[:2]
        graphs = len(eng._graphs)
    finally:
        eng.stop()
    assert alone.prompt_lp[0] is None and len(alone.prompt_lp) == len(prompt)
    assert batched.prompt_lp == alone.prompt_lp  # bit for bit, whatever shares the steps and however they are cut

    cfg = eng.model.cfg
    z, bz = reference(x, head.float(), scale, cfg.eps, cfg.dim)
    lse, b_lse = lse_bound(z, bz)
    worst = 0.0
    for p in range(len(prompt) - 1):
        lp, top_id, top_lp = alone.prompt_lp[p + 1]
        t = prompt[p + 1] % cfg.vocab
        worst = max(worst, abs(lp - (z[p, t] - lse[p]).item()) / (bz[p, t] + b_lse[p]).item(),
                    abs(top_lp - (z[p].max() - lse[p]).item()) / (bz[p].max() + b_lse[p]).item())
    print(f"engine prompt logprobs: largest error / bound {worst}")
    assert worst <= 1.0

    plain = Engine(config="tiny", max_batch=4, weight_dtype=weight_dtype)
    try:
        assert run(plain, [Request(p1, 6), Request(p2, 6)]) == gen  # greedy tokens as without the switch
        assert len(plain._graphs) == graphs
        # Independent of resid: the step's own LM head and k_logprobs. A request that ends at prompt row k samples
        # there, so its first token and that token's logprob are row k's top token and top logprob, from bf16 logits:
        # each logit within 2^-9 |z| of its fp32 value, and so are their maximum and their log-sum-exp. Rows 19 and
        # 29 emitted nothing in the scoring run: the 64-row graph's LM head never saw them there.
        for k in (19, 29, 39):
            r = Request(prompt[:k + 1], 1, logprobs=0)
            (tok,), = run(plain, [r])
            tol = 2 * 2.0 ** -9 * z[k].abs().max().item() + (bz[k].max() + b_lse[k]).item()
            if k + 1 < len(prompt):
                _, top_id, top_lp = alone.prompt_lp[k + 1]
                top2 = z[k].topk(2).values
                assert tok == top_id or (top2[0] - top2[1]).item() <= tol
            else:  # the last prompt row has no record: the reference stands in
                top_lp = (z[k].max() - lse[k]).item()
            print(f"row {k}: |step's logprob - scored top logprob| {abs(r.lp[0][0] - top_lp)}, tolerance {tol}")
            assert abs(r.lp[0][0] - top_lp) <= tol
    finally:
        plain.stop()
