"""Numerics of the gfx950 HIP kernels vs plain fp32 PyTorch references.

All tests need an MI355X (``-m gpu``). They also assert that the kernels ran
from the in-tree ``_hip_ops.so`` (no silent fallback exists).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

cuda = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")


@pytest.fixture(scope="module")
def ops():
    from p2p_llm_tunnel_amd import ops as o
    o.lib()
    return o


def bf(x):
    return x.to(torch.bfloat16)


def close(a, b, tol):
    err = (a.float() - b.float()).abs().max().item()
    scale = b.float().abs().max().item() + 1e-6
    assert err <= tol * scale, f"max err {err} vs scale {scale}"


@cuda
@pytest.mark.parametrize("rows,hidden", [(1, 1024), (7, 4096), (33, 8192), (4, 256), (2, 16384)])
def test_rmsnorm(ops, rows, hidden):
    torch.manual_seed(0)
    x = bf(torch.randn(rows, hidden, device="cuda"))
    w = bf(1 + 0.1 * torch.randn(hidden, device="cuda"))
    ref = x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6) * w.float()
    close(ops.rmsnorm(x, w, 1e-6), ref, 1e-2)


@cuda
def test_rmsnorm_fused_residual(ops):
    torch.manual_seed(1)
    x = bf(torch.randn(9, 2048, device="cuda"))
    r = bf(torch.randn(9, 2048, device="cuda"))
    w = bf(torch.ones(2048, device="cuda"))
    out, res = ops.rmsnorm(x, w, 1e-5, residual=r)
    s = (x.float() + r.float()).to(torch.bfloat16).float()
    assert torch.equal(res.float(), s)
    close(out, s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + 1e-5), 1e-2)


@cuda
@pytest.mark.parametrize("rows,F", [(1, 2816), (16, 5632), (3, 8)])
def test_silu_mul(ops, rows, F):
    torch.manual_seed(2)
    gu = bf(torch.randn(rows, 2 * F, device="cuda") * 3)
    ref = torch.nn.functional.silu(gu[:, :F].float()) * gu[:, F:].float()
    close(ops.silu_mul(gu), ref, 1e-2)


def rope_ref(x, pos, D, theta):
    half = D // 2
    inv = torch.exp2(-math.log2(theta) * torch.arange(half, device=x.device, dtype=torch.float32) * 2 / D)
    ang = pos.float()[:, None, None] * inv[None, None, :]
    c, s = torch.cos(ang), torch.sin(ang)
    x1, x2 = x[..., :half].float(), x[..., half:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


@cuda
@pytest.mark.parametrize("D", [64, 128])
def test_rope_qkv_cache(ops, D):
    torch.manual_seed(3)
    B, H, Hkv, Smax = 5, 8, 2, 300
    qkv = bf(torch.randn(B, (H + 2 * Hkv) * D, device="cuda"))
    pos = torch.tensor([0, 1, 17, 150, 299], dtype=torch.int32, device="cuda")
    kc = torch.zeros(B, Smax, Hkv, D, dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    q = ops.rope_qkv_cache(qkv, pos, kc, vc, H, Hkv, D)
    qr = rope_ref(qkv[:, : H * D].view(B, H, D), pos, D, 10000.0)
    kr = rope_ref(qkv[:, H * D:(H + Hkv) * D].view(B, Hkv, D), pos, D, 10000.0)
    close(q, qr, 1e-2)
    bidx = torch.arange(B, device="cuda")
    close(kc[bidx, pos.long()], kr, 1e-2)
    assert torch.equal(vc[bidx, pos.long()], qkv[:, (H + Hkv) * D:].view(B, Hkv, D))
    # untouched positions stay zero
    assert kc[0, 1:].abs().sum().item() == 0


def attn_ref(q, kc, vc, lens):
    B, H, D = q.shape
    Hkv = kc.shape[2]
    G = H // Hkv
    out = torch.empty(B, H, D, device=q.device)
    for b in range(B):
        L = int(lens[b])
        k = kc[b, :L].float().repeat_interleave(G, dim=1)  # [L, H, D]
        v = vc[b, :L].float().repeat_interleave(G, dim=1)
        s = torch.einsum("hd,lhd->hl", q[b].float(), k) / math.sqrt(D)
        out[b] = torch.einsum("hl,lhd->hd", s.softmax(-1), v)
    return out


@cuda
@pytest.mark.parametrize("D,H,Hkv", [(64, 16, 4), (128, 32, 8), (128, 8, 1), (64, 8, 8)])
@pytest.mark.parametrize("chunk", [64, 256])
def test_decode_attention(ops, D, H, Hkv, chunk):
    torch.manual_seed(4)
    B, Smax = 4, 1100
    q = bf(torch.randn(B, H, D, device="cuda"))
    kc = bf(torch.randn(B, Smax, Hkv, D, device="cuda"))
    vc = bf(torch.randn(B, Smax, Hkv, D, device="cuda"))
    lens = torch.tensor([1, 63, 700, 1100], dtype=torch.int32, device="cuda")
    out = ops.decode_attention(q, kc, vc, lens, chunk=chunk)
    close(out, attn_ref(q, kc, vc, lens), 2e-2)


@cuda
@pytest.mark.parametrize("V", [32000, 4096, 1001])
def test_argmax(ops, V):
    torch.manual_seed(5)
    x = bf(torch.randn(6, V, device="cuda"))
    x[2, 5] = 100.0
    x[3, :] = 1.0  # all ties -> first index
    got = ops.argmax(x)
    assert torch.equal(got, x.float().argmax(-1))
    assert got[3].item() == 0


@cuda
@pytest.mark.parametrize("M,N,K", [(1, 1536, 1024), (8, 2048, 2816), (16, 32000, 1024), (3, 64, 256), (16, 96, 4096),
                                   (5, 256, 96), (16, 64, 8192),
                                   # several 16-row MFMA tiles (blockIdx.y), partial last tile
                                   (17, 1536, 1024), (40, 2048, 2816), (64, 32000, 1024), (33, 96, 4096)])
def test_skinny_gemm(ops, M, N, K):
    # Asymmetric operands: a transposed C write would not pass.
    torch.manual_seed(M * 7 + K)
    x = bf(torch.randn(M, K, device="cuda"))
    w = bf(torch.randn(N, K, device="cuda") / math.sqrt(K))
    got = ops.skinny_gemm(x, w)
    ref = x.float() @ w.float().T
    err = (got.float() - ref).abs().max().item()
    assert err <= 0.01 * ref.abs().max().item() + 1e-3, err
    # exact-integer check of the fragment layout (row/col mapping)
    xi = bf(torch.randint(-3, 4, (M, K), device="cuda").float())
    wi = bf(torch.randint(-3, 4, (N, K), device="cuda").float())
    ref_i = (xi.float() @ wi.float().T)
    got_i = ops.skinny_gemm(xi, wi).float()
    exact = ref_i.abs() <= 256  # bf16 represents these integers exactly
    assert torch.equal(got_i[exact], ref_i[exact])


@cuda
def test_host_side_shape_checks(ops):
    q = bf(torch.randn(2, 8, 64, device="cuda"))
    kc = bf(torch.randn(2, 10, 2, 64, device="cuda"))
    with pytest.raises(ValueError):
        ops.decode_attention(q, kc, kc, torch.tensor([5, 11], dtype=torch.int32, device="cuda"))  # > Smax
    with pytest.raises(TypeError):
        ops.argmax(torch.randn(2, 10, device="cuda"))  # fp32
    with pytest.raises(ValueError):
        ops.rope_qkv_cache(bf(torch.randn(2, 5, device="cuda")), torch.zeros(2, dtype=torch.int32, device="cuda"),
                           kc, kc, 8, 2, 64)
    with pytest.raises(ValueError):
        ops.skinny_gemm(bf(torch.randn(65, 128, device="cuda")), bf(torch.randn(32, 128, device="cuda")))  # M > 64
    with pytest.raises(ValueError):
        ops.skinny_gemm(bf(torch.randn(2, 100, device="cuda")), bf(torch.randn(32, 100, device="cuda")))  # K % 32


@cuda
def test_native_library_is_loaded(ops):
    import os
    path = ops.loaded_path()
    assert os.path.exists(path)
    with open("/proc/self/maps") as f:
        assert "_hip_ops.so" in f.read()


def _ref_probs(logits_row: torch.Tensor, T: float, k: int, p: float) -> torch.Tensor:
    """fp32 reference of the sampler's distribution: softmax(z / T) after
    top-k (ties at the k-th value kept) and top-p (the largest tokens until
    their mass reaches p, the crossing token included)."""
    z = logits_row.float() / T
    keep = torch.ones_like(z, dtype=torch.bool)
    if 0 < k < z.numel():
        keep &= z >= torch.topk(z, k).values[-1]
    if p < 1:
        zk = torch.where(keep, z, torch.tensor(-float("inf"), device=z.device))
        pr = torch.softmax(zk, -1)
        order = torch.argsort(pr, descending=True)
        before = torch.cumsum(pr[order], 0) - pr[order]
        # The cut is a value: every token whose z equals that of the last one
        # needed to reach p is kept too (the kernel keeps z >= z_(p)). bf16
        # logits tie often at V = 32,000, and an order-based cut kept an
        # arbitrary part of the tied tokens.
        cut = zk[order][before < p].min()
        keep &= zk >= cut
    zf = torch.where(keep, z, torch.tensor(-float("inf"), device=z.device))
    return torch.softmax(zf, -1)


def _draws(ops, row, T, k, p, n_launch=200, B=64, seed=1234):
    logits = row.expand(B, -1).contiguous()
    out = []
    for j in range(n_launch):
        ids = torch.zeros(B, dtype=torch.int64, device="cuda")
        params = torch.tensor([ops.pack_sampling(T, k, p, seed, j * B + b) for b in range(B)],
                              dtype=torch.int64, device="cuda").T.contiguous()
        ops.sample_(logits, ids, params)
        out.append(ids)
    return torch.cat(out)


@cuda
@pytest.mark.parametrize("V,scale,T,k,p", [
    (1000, 2.0, 0.8, 0, 1.0), (1000, 2.0, 1.0, 20, 1.0), (1000, 2.0, 0.7, 0, 0.9), (1000, 2.0, 1.2, 50, 0.8),
    (1000, 2.0, 1.0, 0, 0.5),
    # Real vocab sizes: the radix-select top-k / top-p passes over 32,000 logits.
    (32000, 2.0, 1.0, 50, 0.9), (32000, 4.0, 0.8, 0, 0.9), (32000, 3.0, 1.0, 50, 1.0)])
def test_sample_matches_reference_distribution(ops, V, scale, T, k, p):
    """12,800 draws from one logits row vs the fp32 reference distribution:
    a chi-square test (bins of expected count >= 5, the rest pooled) at the
    0.01 % level, and no draw outside the kept set. (Over 20 seeds per case
    the p-values are uniform — mean 0.43-0.49: profiles/r03/sample_diag.json.
    The host replay of the hash that reproduces every draw is
    tests/test_gpu_sample.py, which compares ids, not histograms.)"""
    from scipy.stats import chi2
    torch.manual_seed(11)
    row = bf(torch.randn(V, device="cuda") * scale)
    probs = _ref_probs(row, T, k, p).double().cpu()
    got = _draws(ops, row, T, k, p).cpu()
    n = got.numel()
    assert (probs[got] > 0).all(), "a draw outside the top-k / top-p set"
    counts = torch.bincount(got, minlength=V).double()
    exp = probs * n
    big = exp >= 5
    obs_b, exp_b = counts[big], exp[big]
    rest_o, rest_e = counts[~big].sum(), exp[~big].sum()
    stat = ((obs_b - exp_b) ** 2 / exp_b).sum().item()
    dof = int(big.sum().item()) - 1
    if rest_e >= 5:
        stat += ((rest_o - rest_e) ** 2 / rest_e).item()
        dof += 1
    assert dof >= 1
    assert stat < chi2.ppf(0.9999, dof), (stat, dof)


@cuda
def test_sample_greedy_rows_untouched_and_seeded_draws_reproduce(ops):
    torch.manual_seed(3)
    B, V = 8, 32000
    logits = bf(torch.randn(B, V, device="cuda"))
    greedy = ops.argmax(logits)
    cols = [ops.pack_sampling(0.0, 0, 1.0, 7, b) for b in range(4)] + \
           [ops.pack_sampling(0.9, 40, 0.95, 7, b) for b in range(4)]
    params = torch.tensor(cols, dtype=torch.int64, device="cuda").T.contiguous()
    a = greedy.clone()
    ops.sample_(logits, a, params)
    assert torch.equal(a[:4], greedy[:4])  # T = 0: the fused argmax stands, bit-exact
    b = greedy.clone()
    ops.sample_(logits, b, params)
    assert torch.equal(a, b)  # same seed and counters: the same draws
    # top_k = 1 is greedy whatever the temperature (a unique maximum per row)
    logits[torch.arange(B), torch.arange(B) * 1000 + 17] = 12.0
    greedy = ops.argmax(logits)
    one = torch.tensor([ops.pack_sampling(1.5, 1, 1.0, 9, b) for b in range(B)], dtype=torch.int64,
                       device="cuda").T.contiguous()
    c = torch.zeros(B, dtype=torch.int64, device="cuda")
    ops.sample_(logits, c, one)
    assert torch.equal(c, greedy)
