"""Per-layer, per-KV-head scales of the FP8 KV cache, the host side: ``KvScales`` and ``--kv-scales``, the plans of
a model without scales, the checkpoint loader, the calibrator's reduction, the fp32 reference, and a NumPy emulation
of the scaled store and the scaled attention (``utils/kv_fp8_ref.py``) held to fp64. No GPU.

The emulation's checks are the GPU tests' (tests/test_gpu_kv_scale.py). With power-of-two scales x * fp32(1 / s) is
exact, so every stored byte must be RNE(clamp(x / s)) of the fp64 value (``rne64``, e_pre = 0: nothing is
undecided), and attention must stay within ``stage_attn``'s bound of the fp64 attention over decode(byte) * s: a
power-of-two k_scale in the score scale and v_scale in place of 1 in the final division add no rounding, so the
bound of the unscaled stage holds as it stands. Each one-line slip changes a byte or leaves that bound.
"""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models import kv_scales as kvs
from p2p_llm_tunnel_amd.models import server
from p2p_llm_tunnel_amd.models.checkpoint import load_llama
from p2p_llm_tunnel_amd.models.kv_scales import KvScales
from p2p_llm_tunnel_amd.models.tiny_llm import CONFIGS, LlamaConfig, TinyLlama
from p2p_llm_tunnel_amd.utils import kv_fp8_ref as ref
from test_gpu_fused_stages import BF, stage_attn, worst
from test_kv_fp8 import FAMILIES, dims, flat, rne64
from test_qwen2_checkpoint import HKV, NL, _tensors, _write

MICRO = CONFIGS["micro"]  # 2 layers, 2 KV heads


# ---------------------------------------------------------------- the value type
def test_kv_scales_validation_and_each_refusal():
    s = KvScales([[1.0, 2.0], [0.5, 4.0]], [[1, 1], [1, 1]])
    assert s.k.dtype == torch.float32 and tuple(s.k.shape) == (2, 2) and s.k.device.type == "cpu"
    assert s.check(2, 2, "fp8") is s
    with pytest.raises(ValueError, match=r"need kv_dtype='fp8' \(--kv-dtype fp8\): a bf16 KV cache has no scales"):
        s.check(2, 2, "bf16")
    with pytest.raises(ValueError, match=r"shape \(2, 2\), but the model has \(n_layers, n_kv_heads\) = \(4, 2\)"):
        s.check(4, 2)
    with pytest.raises(ValueError, match=r"\(n_layers, n_kv_heads\) = \(2, 4\)"):
        s.check(2, 4)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="kv_scales.k entries must be finite and > 0"):
            KvScales([[1.0, bad]], [[1.0, 1.0]])
        with pytest.raises(ValueError, match="kv_scales.v entries must be finite and > 0"):
            KvScales([[1.0, 1.0]], [[bad, 1.0]])
    with pytest.raises(ValueError, match="finite fp32 reciprocal"):
        KvScales([[1e-45]], [[1.0]])
    with pytest.raises(ValueError, match="k has shape"):
        KvScales([[1.0, 1.0]], [[1.0]])
    with pytest.raises(ValueError, match=r"must be \[n_layers\]\[n_kv_heads\]"):
        KvScales([1.0, 1.0], [1.0, 1.0])
    with pytest.raises(ValueError, match="must be numbers"):
        KvScales([["a"]], [[1.0]])
    # the device table: the reciprocals are fp32(1 / s), computed on the host, then the scales themselves
    t = KvScales([[3.0, 2.0]], [[0.25, 7.0]]).table("cpu")
    assert tuple(t.shape) == (4, 1, 2) and t.dtype == torch.float32
    assert t[0, 0, 0].item() == np.float32(1) / np.float32(3) and t[1, 0, 0].item() == 4.0
    assert t[2].tolist() == [[3.0, 2.0]] and t[3].tolist() == [[0.25, 7.0]]
    assert np.array_equal(ref.recip([3.0, 2.0]), t[0, 0].numpy())


def test_json_round_trip_and_file_refusals(tmp_path):
    s = KvScales([[2.0 ** -3, 0.3], [16.0, 1.0]], [[1.5, 2.0], [2.0 ** -10, 3.0]])
    assert KvScales.from_json(s.to_json()) == s and KvScales.from_json(s.to_json()) != KvScales(s.v, s.k)
    f = tmp_path / "s.json"
    s.save(str(f))
    assert set(json.loads(f.read_text())) == {"k", "v"}
    assert KvScales.load(str(f)) == s and kvs.parse_kv_scales(str(f)) == s
    assert kvs.parse_kv_scales(None, "bf16") is None and kvs.parse_kv_scales("checkpoint") == "checkpoint"
    assert kvs.parse_kv_scales(s) is s
    with pytest.raises(ValueError, match="not JSON"):
        KvScales.from_json("{k:")
    with pytest.raises(ValueError, match=r'must be \{"k": \[\[...\]\], "v": \[\[...\]\]\}'):
        KvScales.from_json('{"k": [[1]]}')
    with pytest.raises(ValueError, match="cannot read"):
        kvs.parse_kv_scales(str(tmp_path / "missing.json"))
    with pytest.raises(ValueError, match="a bf16 KV cache has no scales"):
        kvs.parse_kv_scales(str(f), "bf16")
    with pytest.raises(ValueError, match="must be a KvScales, 'checkpoint' or the path"):
        kvs.parse_kv_scales(3)


def test_the_switch_and_its_refusal_with_a_bf16_cache(tmp_path):
    ap = server.arg_parser()
    assert ap.parse_args([]).kv_scales is None
    assert ap.parse_args(["--kv-dtype", "fp8", "--kv-scales", "checkpoint"]).kv_scales == "checkpoint"
    f = tmp_path / "s.json"
    KvScales([[1.0, 2.0]] * 2, [[1.0, 2.0]] * 2).save(str(f))
    with pytest.raises(SystemExit, match="--kv-scales needs --kv-dtype fp8"):
        server.main(["--kv-scales", str(f)])
    with pytest.raises(SystemExit, match="--kv-scales needs --kv-dtype fp8"):
        server.main(["--kv-scales", "checkpoint", "--kv-dtype", "bf16", "--gpus", "2"])
    with pytest.raises(ValueError, match="a bf16 KV cache has no scales"):
        server.start_server(kv_scales=str(f))
    with pytest.raises(ValueError, match="needs a checkpoint to read them from"):
        server.start_server(kv_dtype="fp8", kv_scales="checkpoint")
    # --gpus N passes it on
    a = ap.parse_args(["--gpus", "2", "--kv-dtype", "fp8", "--kv-scales", str(f), "--port", "9000"])
    for i in range(2):
        cmd = server.replica_cmd(a, i)
        assert cmd[cmd.index("--kv-scales") + 1] == str(f) and cmd[cmd.index("--kv-dtype") + 1] == "fp8"
    assert "--kv-scales" not in server.replica_cmd(ap.parse_args(["--gpus", "2", "--kv-dtype", "fp8"]), 0)


def test_model_engine_and_decoder_refusals():
    s = KvScales([[1.0, 2.0]] * 2, [[4.0, 0.5]] * 2)
    m = TinyLlama(MICRO, device="cpu", max_batch=2, kv_dtype="fp8", kv_scales=s)
    assert m.kv_scales is s and TinyLlama(MICRO, device="cpu", max_batch=2, kv_dtype="fp8").kv_scales is None
    with pytest.raises(ValueError, match="a bf16 KV cache has no scales"):
        TinyLlama(MICRO, device="cpu", max_batch=2, kv_scales=s)
    with pytest.raises(ValueError, match=r"the model has \(n_layers, n_kv_heads\) = \(2, 2\)"):
        TinyLlama(MICRO, device="cpu", max_batch=2, kv_dtype="fp8", kv_scales=KvScales([[1.0]], [[1.0]]))
    with pytest.raises(TypeError, match="must be a KvScales"):
        TinyLlama(MICRO, device="cpu", max_batch=2, kv_dtype="fp8", kv_scales={"k": [[1.0]]})
    with pytest.raises(ValueError, match="a bf16 KV cache has no scales"):
        server.Engine(model=TinyLlama(MICRO, device="cpu", max_batch=2), kv_scales=s)
    with pytest.raises(ValueError, match="other scales or none"):
        server.Engine(model=TinyLlama(MICRO, device="cpu", max_batch=2, kv_dtype="fp8"), kv_dtype="fp8", kv_scales=s)
    # the start-up line names the scales and their range
    line = server.kv_cache_line(m, "fp8")
    assert "scales in use: k_scale 1 .. 2, v_scale 0.5 .. 4 per layer and KV head" in line
    assert "scales" not in server.kv_cache_line(TinyLlama(MICRO, device="cpu", max_batch=2, kv_dtype="fp8"), "fp8")
    # the decoder: no scales for a bf16 cache, and the table's shape
    bf = torch.zeros(2, 3, 64, 2, 64, dtype=torch.bfloat16)
    f8 = torch.zeros(2, 3, 64, 2, 64, dtype=torch.float8_e4m3fn)
    d0, d1 = dims(0, H=4, max_seq=64, max_batch=3), dims(1, H=4, max_seq=64, max_batch=3)
    with pytest.raises(ValueError, match="a bf16 KV cache has no scales"):
        ops.FusedLlamaDecoder(d0, [], bf, bf, kv_scales=s.table("cpu"))
    with pytest.raises(ValueError, match=r"kv_scales must be fp32 \[4, 2, 2\]"):
        ops.FusedLlamaDecoder(d1, [], f8, f8, kv_scales=torch.ones(2, 2, 2))
    with pytest.raises(ValueError, match=r"kv_scales must be fp32 \[4, 2, 2\]"):
        ops.FusedLlamaDecoder(d1, [], f8, f8, kv_scales=torch.ones(4, 2, 2, dtype=torch.float64))


# ---------------------------------------------------------------- the plans
def ws_layout(d):
    import ctypes
    n = len(ops.FusedLlamaDecoder._WS_BUFFERS)
    off, cnt = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
    assert ops.lib().p2pt_llama_ws_layout(ctypes.byref(d), off, cnt, n) == n
    return list(off), list(cnt), ops.lib().p2pt_llama_ws_bytes(ctypes.byref(d))


def weight_layout(d, w8):
    import ctypes
    n = 13 * d.n_layers
    idx, sc = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    wp = ops.WeightPlan(w8=w8)
    size = ops.lib().p2pt_llama_weight_layout(ctypes.byref(d), ctypes.byref(wp), idx, sc, n)
    return size, list(idx), list(sc)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_scales_are_no_part_of_dims_plans_table_or_workspace(family):
    # The scales travel beside the plans: LlamaDims has no field for them, so every LlamaDims-derived output of a
    # model, with scales or without, is what a LlamaDims built by hand without any notion of scales gives.
    assert [n for n, _ in ops.LlamaDims._fields_][-4:] == ["kv_fp8", "rope_table", "qk_norm", "qkv_bias"]
    assert len(ops.LlamaDims._fields_) == 15 and [n for n, _ in ops.KvPlan._fields_] == ["attn_kv8", "qk_norm_kv8"]
    from p2p_llm_tunnel_amd.models.rope import RopeScaling
    fam = FAMILIES[family]
    cfg = LlamaConfig(vocab=512, dim=256, n_layers=2, n_heads=8, n_kv_heads=2, head_dim=64, ffn=512, max_seq=256,
                      eps=1e-5, rope_theta=1e4, qk_norm=bool(fam.get("qk_norm")), qkv_bias=bool(fam.get("qkv_bias")),
                      rope_scaling=RopeScaling("llama3", 8.0, 1.0, 4.0, 64) if fam.get("rope_table") else None)
    s = KvScales([[0.5, 2.0], [4.0, 8.0]], [[1.0, 2.0], [0.25, 16.0]])
    plain = TinyLlama(cfg, device="cpu", max_batch=4, kv_dtype="fp8")
    scaled = TinyLlama.from_weights(cfg, dict(embed=plain.embed, final_norm=plain.final_norm, lm_head=plain.lm_head,
                                              layers=plain.layers), device="cpu", max_batch=4, kv_dtype="fp8",
                                    kv_scales=s)
    by_hand = dims(1, **fam)  # max_batch 5 = 4 slots and the scratch slot
    for m in (plain, scaled):
        d = m.dims()
        assert bytes(d) == bytes(by_hand)
        for B in (1, 16, 17, 64):
            assert flat(ops.step_plan(d, B)) == flat(ops.step_plan(by_hand, B))
        assert flat(ops.kv_plan(d)) == flat(ops.kv_plan(by_hand))
        assert ws_layout(d) == ws_layout(by_hand)
        for w8 in (0, 1):
            assert weight_layout(d, w8) == weight_layout(by_hand, w8)
            assert list(ops.WeightTable(d, bool(w8))) == list(ops.WeightTable(by_hand, bool(w8)))
    a, b = plain.fused_weights(), scaled.fused_weights()
    assert len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.float(), y.float()) for x, y in zip(a, b))


# ---------------------------------------------------------------- the loader
def test_loader_reads_the_checkpoints_scales(tmp_path):
    ts = _tensors()
    for i in range(NL):
        p = f"model.layers.{i}.self_attn."
        ts[p + "k_scale"] = torch.tensor(0.5 * (i + 1))  # a scalar
        ts[p + "v_scale"] = torch.tensor([0.125 * (i + 3)])  # shape [1]
    _write(tmp_path, ts)
    m = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64, kv_dtype="fp8", kv_scales="checkpoint")
    assert m.kv_scales.k.tolist() == [[0.5] * HKV, [1.0] * HKV] and m.kv_scales.v.tolist() == [[0.375] * HKV, [0.5] * HKV]
    # without the switch the tensors are not read, as before
    assert load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64, kv_dtype="fp8").kv_scales is None
    with pytest.raises(ValueError, match="a bf16 KV cache has no scales"):
        load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64, kv_scales="checkpoint")
    # a given KvScales wins over nothing and is held to the model's shape
    given = KvScales([[1.0] * HKV] * NL, [[2.0] * HKV] * NL)
    assert load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64, kv_dtype="fp8",
                      kv_scales=given).kv_scales is given
    with pytest.raises(ValueError, match=r"\(n_layers, n_kv_heads\)"):
        load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64, kv_dtype="fp8", kv_scales=KvScales([[1.0]], [[1.0]]))


def test_loader_refuses_a_layer_without_scales_and_takes_kv_scale_for_both(tmp_path):
    ts = _tensors()
    ts["model.layers.0.self_attn.k_scale"] = torch.tensor(0.5)
    ts["model.layers.0.self_attn.v_scale"] = torch.tensor(0.25)
    ts["model.layers.1.self_attn.k_scale"] = torch.tensor(0.5)  # layer 1 has no v_scale
    _write(tmp_path, ts)
    with pytest.raises(ValueError, match=r"the checkpoint has no model\.layers\.1\.self_attn\.v_scale"):
        load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64, kv_dtype="fp8", kv_scales="checkpoint")
    ts = _tensors()
    for i in range(NL):
        ts[f"model.layers.{i}.self_attn.kv_scale"] = torch.tensor([2.0 ** (i - 2)])
    _write(tmp_path, ts)
    m = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64, kv_dtype="fp8", kv_scales="checkpoint")
    assert m.kv_scales.k.tolist() == m.kv_scales.v.tolist() == [[0.25] * HKV, [0.5] * HKV]
    ts["model.layers.0.self_attn.kv_scale"] = torch.tensor([1.0, 2.0, 3.0])
    _write(tmp_path, ts)
    with pytest.raises(ValueError, match=r"expected a scalar, shape \[1\] or \[2\], got 3 values"):
        load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64, kv_dtype="fp8", kv_scales="checkpoint")
    ts["model.layers.0.self_attn.kv_scale"] = torch.tensor(0.0)
    _write(tmp_path, ts)
    with pytest.raises(ValueError, match="finite and > 0"):
        load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64, kv_dtype="fp8", kv_scales="checkpoint")


# ---------------------------------------------------------------- the calibrator's reduction
def test_calibrator_reduction_on_hand_built_caches():
    L, slots, S, Hkv, D = 2, 3, 16, 2, 64
    g = torch.Generator().manual_seed(1)
    kc = (torch.randn(L, slots, S, Hkv, D, generator=g) * 0.5).to(BF)
    vc = (torch.randn(L, slots, S, Hkv, D, generator=g) * 0.5).to(BF)
    lengths = [5, 0, 9]
    kc[1, 2, 8, 0, 17] = -3072.0  # the absmax of K: layer 1, head 0, the last written row of slot 2
    vc[0, 0, 0, 1, 3] = 100.0  # ... and of V: layer 0, head 1
    kc[0, 2, 9, 1, 0] = 1e6  # first row past slot 2's length: not written, does not count
    kc[1, 1, 0, 1, 0] = 1e6  # slot 1 holds nothing
    vc[1, 0, 5, 0, 0] = -1e6
    ka, va = kvs.absmax(kc, vc, lengths)
    assert tuple(ka.shape) == (L, Hkv) and ka[1, 0].item() == 3072.0 and va[0, 1].item() == 100.0
    assert ka.max().item() == 3072.0 and va.max().item() == 100.0 and (ka.argmax().item(), va.argmax().item()) == (2, 1)
    others = torch.tensor([ka[0, 0], ka[0, 1], ka[1, 1], va[0, 0], va[1, 0], va[1, 1]])
    assert bool((others < 4.0).all()) and bool((others > 0.5).all())
    s = kvs.scales_from_absmax(ka, va)
    assert kvs.is_power_of_two(s.k) and kvs.is_power_of_two(s.v)
    for sc, am in ((s.k, ka), (s.v, va)):
        assert bool((sc.double() >= am.double() / 448).all()) and bool((sc.double() < 2 * am.double() / 448).all())
    assert s.k[1, 0].item() == 8.0 and s.v[0, 1].item() == 0.25  # 3072 / 448 = 6.9 -> 8; 100 / 448 = 0.22 -> 0.25
    # exact powers of two stay; an all-zero head gets scale 1; more slots than the cache has are refused
    s2 = kvs.scales_from_absmax(torch.tensor([[448.0, 0.0]]), torch.tensor([[224.0, 449.0]]))
    assert s2.k.tolist() == [[1.0, 1.0]] and s2.v.tolist() == [[0.5, 2.0]]
    with pytest.raises(ValueError, match="lengths"):
        kvs.absmax(kc, vc, [1, 1, 1, 1])
    with pytest.raises(ValueError, match="non-finite"):
        kvs.scales_from_absmax(torch.tensor([[float("inf")]]), torch.tensor([[1.0]]))


# ---------------------------------------------------------------- the fp32 reference
def test_reference_with_scales():
    cfg = LlamaConfig(vocab=512, dim=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=256, max_seq=64,
                      qkv_bias=True)
    base = TinyLlama(cfg, device="cpu", max_batch=1, seed=5)
    for L in base.layers:  # K of a few thousand in KV head 1, as Qwen2-family biases can be; its q heads (2, 3) as
        # much smaller, so the scores stay a few units and e4m3's relative error does not decide the softmax by itself
        for name in ("wqkv", "bqkv"):
            L[name][(4 + 1) * 64:(4 + 2) * 64] = (L[name][(4 + 1) * 64:(4 + 2) * 64].float() * 1024).to(BF)
            L[name][2 * 64:4 * 64] = (L[name][2 * 64:4 * 64].float() / 1024).to(BF)
    w = dict(embed=base.embed, final_norm=base.final_norm, lm_head=base.lm_head, layers=base.layers)
    mk = lambda **kw: TinyLlama.from_weights(cfg, w, device="cpu", max_batch=1, **kw)
    seq = torch.arange(7, 31)[None]
    bf16, fp8 = mk().reference_logits(seq), mk(kv_dtype="fp8").reference_logits(seq)
    ones = KvScales(torch.ones(2, 2), torch.ones(2, 2))
    assert torch.equal(mk(kv_dtype="fp8", kv_scales=ones).reference_logits(seq), fp8)  # scale 1: bit for bit
    s = KvScales([[1.0, 16.0], [1.0, 16.0]], [[1.0, 1.0], [1.0, 1.0]])
    scaled = mk(kv_dtype="fp8", kv_scales=s).reference_logits(seq)
    top = bf16.abs().max().item()
    # at scale 1 head 1's K saturates and the logits are another model's; with the scale they are FP8-close to bf16
    assert (fp8 - bf16).abs().max().item() > 0.05 * top > (scaled - bf16).abs().max().item()
    # an explicit kv_round is used as given: the scales belong to the model's own format only
    assert torch.equal(mk(kv_dtype="fp8", kv_scales=s).reference_logits(seq, kv_round=lambda t: t.to(BF).float()), bf16)


# ---------------------------------------------------------------- NumPy emulation of the scaled store and read
NL_, NHKV, G_, D_ = 2, 2, 2, 64
K_SCALE = np.float32([[2.0 ** -3, 2.0 ** 1], [2.0 ** 4, 2.0 ** -1]])  # differ per head, per layer and from V's
V_SCALE = np.float32([[2.0 ** 2, 2.0 ** -2], [2.0 ** -4, 2.0 ** 3]])
ROWS = ((0, 39, 1), (1, 199, 4))  # (cache slot, position, span slots): the single-slot exit and the merge
STORE_SLIPS = ("v_scale_dropped", "k_scale_for_v", "layer0_row_for_layer1", "head0_for_every_head", "times_s")
READ_SLIPS = ("reader_forgets_k_scale", "reader_forgets_v_scale", "v_scale_in_merge_only")


def emu_inputs():
    """fp32 K and V rows [L, slots, S, Hkv, D] of magnitude about 3 s (so x / s uses the format's range), and bf16 q
    [rows, Hkv * G, D] small enough for moderate scores against K / s ... times s."""
    rng = np.random.default_rng(11)
    shape = (NL_, 2, 200, NHKV, D_)
    xk = (rng.standard_normal(shape) * 3).astype(np.float32) * K_SCALE[:, None, None, :, None]
    xv = (rng.standard_normal(shape) * 3).astype(np.float32) * V_SCALE[:, None, None, :, None]
    q = torch.from_numpy(rng.standard_normal((NL_, len(ROWS), NHKV * G_, D_)).astype(np.float32))
    q = q / torch.from_numpy(K_SCALE)[:, None, :, None].repeat_interleave(G_, 2)  # scores of a few units
    return xk, xv, (q * 0.5).to(BF)


def emulate(slip=None):
    """{"kb", "vb": bytes [L, slots, S, Hkv, D]; "attn": bf16 [L, rows, H * D]} of the scaled store and read."""
    xk, xv, q = emu_inputs()
    ks, vs = K_SCALE.copy(), V_SCALE.copy()
    wk, wv = ks.copy(), vs.copy()  # what the writers use
    if slip == "v_scale_dropped":
        wv[:] = 1
    elif slip == "k_scale_for_v":
        wv = wk.copy()
    elif slip == "layer0_row_for_layer1":
        wk[1], wv[1] = wk[0], wv[0]
    elif slip == "head0_for_every_head":
        wk[:], wv[:] = wk[:, :1], wv[:, :1]
    elif slip == "times_s":
        wk, wv = 1 / wk, 1 / wv
    kb = np.stack([ref.encode_scaled(xk[l], wk[l]) for l in range(NL_)])
    vb = np.stack([ref.encode_scaled(xv[l], wv[l]) for l in range(NL_)])
    attn = np.zeros((NL_, len(ROWS), NHKV * G_, D_), np.float32)
    for l in range(NL_):
        for r, (slot, pos, slots) in enumerate(ROWS):
            for h in range(NHKV):
                rk = 1.0 if slip == "reader_forgets_k_scale" else ks[l, h]
                rv = 1.0 if slip == "reader_forgets_v_scale" or (slip == "v_scale_in_merge_only" and slots == 1) \
                    else vs[l, h]
                attn[l, r, h * G_:(h + 1) * G_] = ref.attend(
                    q[l, r, h * G_:(h + 1) * G_].float().numpy(), kb[l, slot, :pos + 1, h], vb[l, slot, :pos + 1, h],
                    rk, rv, slots=slots)
    return {"kb": kb, "vb": vb, "attn": torch.from_numpy(attn).to(BF).reshape(NL_, len(ROWS), -1)}


def judge_emulation(out):
    """(stored bytes that are not RNE(x / s) of the fp64 value, the worst attention ratio to ``stage_attn``'s bound
    over the fp64 attention from decode(byte) * s)."""
    xk, xv, q = emu_inputs()
    wrong = 0
    for x, s, b in ((xk, K_SCALE, out["kb"]), (xv, V_SCALE, out["vb"])):
        want = rne64(x.astype(np.float64) / s.astype(np.float64)[:, None, None, :, None])
        wrong += int((want != b).sum())
    cfg = SimpleNamespace(cfg=SimpleNamespace(n_heads=NHKV * G_, n_kv_heads=NHKV, head_dim=D_))
    pos = torch.tensor([p for _, p, _ in ROWS])
    slots = torch.tensor([s for s, _, _ in ROWS])
    ratio = 0.0
    for l in range(NL_):
        kd = torch.from_numpy(ref.decode_scaled(out["kb"][l], K_SCALE[l]))
        vd = torch.from_numpy(ref.decode_scaled(out["vb"][l], V_SCALE[l]))
        ratio = max(ratio, worst(out["attn"][l], stage_attn(cfg, q[l], kd, vd, pos, slots)))
    return wrong, ratio


def test_emulation_of_the_scaled_store_and_read_holds_fp64():
    out = emulate()
    wrong, ratio = judge_emulation(out)
    print("EMU kv-scale", wrong, round(ratio, 4))
    assert wrong == 0 and ratio <= 1.0
    # scale 1 is the unscaled store, byte for byte
    xk, _, _ = emu_inputs()
    assert np.array_equal(ref.encode_scaled(xk[0], np.ones(NHKV, np.float32)), ref.encode(xk[0]))
    # x / s uses the format: nothing saturates, and most values are normal
    mag = out["kb"] & 0x7F
    assert int((mag == 0x7E).sum()) == 0 and float((mag >= 8).mean()) > 0.9
    assert len({*K_SCALE.ravel(), *V_SCALE.ravel()}) == 8


@pytest.mark.parametrize("slip", STORE_SLIPS + READ_SLIPS)
def test_every_slip_changes_a_byte_or_leaves_the_bound(slip):
    wrong, ratio = judge_emulation(emulate(slip))
    print("SLIP kv-scale", slip, wrong, round(ratio, 3))
    if slip in STORE_SLIPS:
        assert wrong > 0, slip
    else:
        assert wrong == 0 and ratio > 1.0, (slip, ratio)
