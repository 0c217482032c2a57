"""Qwen3 checkpoints (models/checkpoint.py: ``Qwen3ForCausalLM``, per-head QK RMSNorm) without a GPU: the name
mapping against transformers' own Qwen3 on a synthetic checkpoint written here, the refusals, what the fused
step plans for a QK-norm model, an fp32 NumPy emulation of ``k_qknorm_rope`` held to the fp64 bound of
tests/test_gpu_qk_norm.py (and six one-line slips that each leave it), the ``chat_template_kwargs`` request
field and the EOS ids of ``generation_config.json``."""
import ctypes
import http.client
import json
import math

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

from p2p_llm_tunnel_amd import ops
from p2p_llm_tunnel_amd.models.checkpoint import Tokenizer, load_llama, read_config
from test_checkpoint import _FakeModel, _tokenizer_dir
from test_gpu_qk_norm import (BF, CASE_IDS, CASES, ENGINE_PROMPTS, EPS, POISON_BITS, QK2, case_reference, check_outputs,
                              inputs, poisoned)

QWEN3 = dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, head_dim=64, max_position_embeddings=512, rms_norm_eps=1e-6, rope_theta=1e6,
             tie_word_embeddings=True)


def qwen3_checkpoint(path, seed=0):
    """A random transformers Qwen3 (H * D = 256 != hidden_size = 128) saved as safetensors, weights rounded to
    bf16 so both sides compute with identical weights; q_norm and k_norm drawn well away from 1."""
    transformers = pytest.importorskip("transformers")
    cfg = transformers.Qwen3Config(**QWEN3)
    torch.manual_seed(seed)
    m = transformers.Qwen3ForCausalLM(cfg).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() > 1:
                p.normal_(0, 0.05)
            elif "q_norm" in name or "k_norm" in name:
                p.uniform_(0.5, 1.5)
            else:
                p.uniform_(0.8, 1.2)
            p.copy_(p.to(torch.bfloat16).float())
    m.save_pretrained(path, safe_serialization=True)
    return m


def hf_logits(m, seqs):
    with torch.no_grad():
        return m(seqs).logits[:, -1].float()


def test_loader_matches_transformers_qwen3(tmp_path):
    m = qwen3_checkpoint(str(tmp_path))
    ours = load_llama(str(tmp_path), device="cpu", max_batch=2)
    c = ours.cfg
    assert (c.vocab, c.dim, c.n_layers, c.n_heads, c.n_kv_heads, c.head_dim, c.ffn) == (512, 128, 2, 4, 2, 64, 256)
    assert c.qk_norm and c.n_heads * c.head_dim != c.dim and c.rope_theta == 1e6 and c.eps == 1e-6
    assert ours.lm_head is ours.embed
    sd = m.state_dict()
    for i, L in enumerate(ours.layers):
        for n in ("q_norm", "k_norm"):
            assert L[n].shape == (64,) and torch.equal(L[n].float(), sd[f"model.layers.{i}.self_attn.{n}.weight"])
    assert not torch.equal(ours.layers[0]["q_norm"], ours.layers[0]["k_norm"])
    torch.manual_seed(3)
    seqs = torch.randint(0, c.vocab, (2, 29))
    ref = ours.reference_logits(seqs)
    hf = hf_logits(m, seqs)
    scale = hf.abs().max().item()
    # the criterion of tests/test_checkpoint.py for Llama: agreement to bf16 accuracy
    assert (ref - hf).abs().max().item() < 0.03 * scale
    assert torch.nn.functional.cosine_similarity(ref, hf, dim=-1).min().item() > 0.999
    # ... which the norm weights decide: swapped, the logits are another model's
    for L in ours.layers:
        L["q_norm"], L["k_norm"] = L["k_norm"], L["q_norm"]
    assert (ours.reference_logits(seqs) - hf).abs().max().item() > 0.03 * scale
    # the fused weight table: 8 entries per layer, wqkv in plain row order with attn_norm folded in
    for L in ours.layers:
        L["q_norm"], L["k_norm"] = L["k_norm"], L["q_norm"]
    table = ours.fused_weights()
    assert len(table) == 3 + 8 * c.n_layers and table[3 + 6] is not None
    assert torch.equal(table[3 + 6], ours.layers[0]["q_norm"]) and torch.equal(table[3 + 7], ours.layers[0]["k_norm"])
    folded = (ours.layers[0]["wqkv"].float() * ours.layers[0]["attn_norm"].float()[None]).to(torch.bfloat16)
    assert torch.equal(table[3 + 1], folded)


# ---------------------------------------------------------------- refusals and neutrality
H, HKV, D, DIM, FFN, V, NL = 4, 2, 64, 128, 256, 512, 2
CONF = {"architectures": ["Qwen3ForCausalLM"], "vocab_size": V, "hidden_size": DIM, "intermediate_size": FFN,
        "num_hidden_layers": NL, "num_attention_heads": H, "num_key_value_heads": HKV, "head_dim": D,
        "max_position_embeddings": 4096, "rms_norm_eps": 1e-6, "rope_theta": 1e6, "tie_word_embeddings": True,
        "layer_types": ["full_attention"] * NL, "use_sliding_window": False, "sliding_window": None}


def _tensors(qk_norm=True):
    g = torch.Generator().manual_seed(0)

    def r(*s):
        return torch.randn(*s, generator=g).to(torch.bfloat16)
    ts = {"model.embed_tokens.weight": r(V, DIM), "model.norm.weight": r(DIM)}
    for i in range(NL):
        p = f"model.layers.{i}."
        ts.update({p + "input_layernorm.weight": r(DIM), p + "post_attention_layernorm.weight": r(DIM),
                   p + "self_attn.q_proj.weight": r(H * D, DIM), p + "self_attn.k_proj.weight": r(HKV * D, DIM),
                   p + "self_attn.v_proj.weight": r(HKV * D, DIM), p + "self_attn.o_proj.weight": r(DIM, H * D),
                   p + "mlp.gate_proj.weight": r(FFN, DIM), p + "mlp.up_proj.weight": r(FFN, DIM),
                   p + "mlp.down_proj.weight": r(DIM, FFN)})
        if qk_norm:
            ts.update({p + "self_attn.q_norm.weight": r(D), p + "self_attn.k_norm.weight": r(D)})
    return ts


def _write(path, tensors, **conf):
    save_file(tensors, str(path / "model.safetensors"))
    (path / "config.json").write_text(json.dumps(dict(CONF, **conf)))


def test_refusals_and_neutrality(tmp_path):
    ts = _tensors()
    _write(tmp_path, ts)
    m = load_llama(str(tmp_path), device="cpu", max_batch=1, max_seq=64)
    assert m.cfg.qk_norm and m.cfg.head_dim == D and m.cfg.n_heads * D != m.cfg.dim
    assert torch.equal(m.layers[1]["k_norm"], ts["model.layers.1.self_attn.k_norm.weight"])
    assert m.k_cache.shape == (NL, 2, 64, HKV, D)

    missing = {k: v for k, v in ts.items() if k != "model.layers.1.self_attn.k_norm.weight"}
    _write(tmp_path, missing)
    with pytest.raises(KeyError, match=r"model\.layers\.1\.self_attn\.k_norm\.weight"):
        load_llama(str(tmp_path), device="cpu", max_seq=64)
    _write(tmp_path, dict(ts, **{"model.layers.0.self_attn.q_norm.weight": torch.ones(H * D, dtype=torch.bfloat16)}))
    with pytest.raises(ValueError, match="q_norm.*shape"):
        load_llama(str(tmp_path), device="cpu", max_seq=64)

    _write(tmp_path, ts)
    for bad, msg in ((dict(architectures=["Qwen3MoeForCausalLM"]), "Qwen3MoeForCausalLM"),
                     (dict(layer_types=["full_attention", "sliding_attention"]), "layer_types.*sliding_attention"),
                     (dict(rope_scaling={"rope_type": "yarn", "factor": 4.0}), "rope"),
                     (dict(attention_bias=True), "bias")):
        (tmp_path / "config.json").write_text(json.dumps(dict(CONF, **bad)))
        with pytest.raises(ValueError, match=msg):
            read_config(str(tmp_path))
    # a sliding window that is switched on keeps capping the context, as for Mistral; switched off it does not
    (tmp_path / "config.json").write_text(json.dumps(dict(CONF, use_sliding_window=True, sliding_window=256)))
    assert read_config(str(tmp_path))[0].max_seq == 256
    (tmp_path / "config.json").write_text(json.dumps(dict(CONF, use_sliding_window=False, sliding_window=256)))
    assert read_config(str(tmp_path))[0].max_seq == 4096

    # A Llama checkpoint carrying q_norm / k_norm is refused, not loaded without them ...
    for arch in ("LlamaForCausalLM", "MistralForCausalLM"):
        _write(tmp_path, ts, architectures=[arch])
        with pytest.raises(ValueError, match="q_norm"):
            load_llama(str(tmp_path), device="cpu", max_seq=64)
    # ... and a plain one loads as before, without the norm.
    _write(tmp_path, _tensors(qk_norm=False), architectures=["LlamaForCausalLM"])
    m = load_llama(str(tmp_path), device="cpu", max_seq=64)
    assert m.cfg.qk_norm is False and "q_norm" not in m.layers[0] and len(m.fused_weights()) == 3 + 6 * NL
    assert read_config(str(tmp_path))[0].qk_norm is False


# ---------------------------------------------------------------- planning (the library, no device)
def _lib_or_skip():
    try:
        return ops.lib()
    except (OSError, RuntimeError) as e:  # no hipcc and no prebuilt library on this host
        pytest.skip(f"the HIP library is not available: {e}")


def _dims(qk_norm, H=16, Hkv=8, D=128, dim=1024, ffn=3072, vocab=151936):
    return ops.LlamaDims(vocab=vocab, dim=dim, n_layers=2, H=H, Hkv=Hkv, D=D, ffn=ffn, max_seq=2048, max_batch=9,
                         eps=1e-6, theta=1e6, qk_norm=qk_norm)


def test_plan_of_a_qk_norm_model():
    lib = _lib_or_skip()
    EPI_STORE, EPI_ROPE = 0, 1
    assert ops.LlamaDims(vocab=1).qk_norm == 0  # every construction without the keyword keeps the old step
    for B in (1, 16, 17, 64):
        on, off = ops.step_plan(_dims(1), B), ops.step_plan(_dims(0), B)
        assert on.qkv.epi == on.qkv_first.epi == EPI_STORE and off.qkv.epi == off.qkv_first.epi == EPI_ROPE
        assert off.qk_norm_grid == 0 and on.qk_norm_grid == 4  # 32 heads of 128: 8 per workgroup
        for name, _ in ops.StepPlan._fields_:  # nothing else moves
            if name in ("qkv", "qkv_first", "qk_norm_grid"):
                continue
            a, b = getattr(on, name), getattr(off, name)
            if isinstance(a, ctypes.Structure):
                a, b = bytes(a), bytes(b)
            assert a == b, (B, name)
        for name, _ in ops.GemmPlan._fields_:
            if name != "epi":
                assert getattr(on.qkv, name) == getattr(off.qkv, name), (B, name)
    # D 64: 16 heads per workgroup; 4 + 2 * 1 = 6 heads fit one, 24 + 2 * 12 = 48 need three
    assert ops.step_plan(_dims(1, H=4, Hkv=1, D=64, dim=256, ffn=256, vocab=512), 3).qk_norm_grid == 1
    assert ops.step_plan(_dims(1, H=24, Hkv=12, D=64, dim=1536, ffn=256, vocab=512), 3).qk_norm_grid == 3
    # The workspace: the qkv buffer comes last and is empty without QK-norm, so that layout stays as it was.
    names = [n for n, _ in ops.FusedLlamaDecoder._WS_BUFFERS]
    assert names[-1] == "qkv"
    n = len(names)
    layouts = {}
    for flag in (0, 1):
        off, cnt = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
        d = _dims(flag)
        assert lib.p2pt_llama_ws_layout(ctypes.byref(d), off, cnt, n) == n
        layouts[flag] = (list(off), list(cnt), lib.p2pt_llama_ws_bytes(ctypes.byref(d)))
    assert layouts[0][0] == layouts[1][0] and layouts[0][1][:-1] == layouts[1][1][:-1]
    assert layouts[0][1][-1] == 0 and layouts[1][1][-1] == 64 * 32 * 128
    assert layouts[0][0][-1] == layouts[0][2] and layouts[1][2] == layouts[0][2] + 64 * 32 * 128 * 2
    bad = _dims(2)
    assert lib.p2pt_llama_ws_bytes(ctypes.byref(bad)) == 0


# ---------------------------------------------------------------- fp32 emulation of the kernel (NumPy)
MUTATIONS = {  # slip -> the outputs of which at least one must leave its bound; the others must stay inside
    "eps_dropped": ("q", "k"), "norm_after_rope": ("q", "k"), "q_weight_for_k": ("k",), "mean_over_half": ("q", "k"),
    "v_normalised": ("v",), "partner_d_plus_1": ("q", "k"),
}


def emulate(case, mut=None):
    """``k_qknorm_rope`` in fp32 NumPy, in the kernel's own order (a lane's four squares, then the xor tree over
    the D / 4 lanes of a head), with its one bf16 rounding; ``mut`` names one slip. Returns (q, k_cache, v_cache)."""
    f32 = np.float32
    inp = inputs(case)
    Hh, Hkv, Dd, R = case.H, case.Hkv, case.D, case.rows
    half, lph = Dd // 2, Dd // 4
    x = inp.qkv.float().numpy().reshape(R, Hh + 2 * Hkv, Dd)
    a, b = x[..., :half].reshape(R, -1, lph, 2), x[..., half:].reshape(R, -1, lph, 2)
    ss = ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + b[..., 0] * b[..., 0]) + b[..., 1] * b[..., 1]
    lanes = np.arange(lph)
    step = 1
    while step < lph:
        ss = ss + ss[..., lanes ^ step]
        step *= 2
    length = Dd // 2 if mut == "mean_over_half" else Dd
    eps = f32(0.0 if mut == "eps_dropped" else EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        rs = (f32(1.0) / np.sqrt(ss[..., :1] * f32(1.0 / length) + eps)).astype(f32)  # [R, heads, 1]
        gq, gk = inp.gq.float().numpy(), inp.gk.float().numpy()
        g = np.stack([gq] * Hh + [gq if mut == "q_weight_for_k" else gk] * Hkv)[None]
        qk, v = x[:, :Hh + Hkv], x[:, Hh + Hkv:]
        i = np.arange(half, dtype=f32)
        inv = np.exp2(-f32(math.log2(case.theta)) * (f32(2.0) * i) / f32(Dd)).astype(f32)
        ang = (inp.pos.numpy().astype(f32)[:, None, None] * inv[None, None, :]).astype(f32)
        cs, sn = np.cos(ang), np.sin(ang)

        def rope(n):
            if mut == "partner_d_plus_1":
                n1, n2 = n[..., 0::2], n[..., 1::2]
                return np.stack([n1 * cs - n2 * sn, n2 * cs + n1 * sn], -1).reshape(n.shape)
            n1, n2 = n[..., :half], n[..., half:]
            return np.concatenate([n1 * cs - n2 * sn, n2 * cs + n1 * sn], -1)

        r = qk * rs[:, :Hh + Hkv]
        o = rope(r) * g if mut == "norm_after_rope" else rope(r * g)
        if mut == "v_normalised":
            v = v * rs[:, Hh + Hkv:]
    assert o.dtype == f32
    o = torch.from_numpy(np.ascontiguousarray(o)).to(BF)
    v = torch.from_numpy(np.ascontiguousarray(v)).to(BF)
    shape = (case.n_slots, case.max_seq, Hkv, Dd)
    kc, vc = poisoned(shape), poisoned(shape)
    s, p = inp.slots.long(), inp.pos.long()
    kc[s, p], vc[s, p] = o[:, Hh:], v
    return o[:, :Hh].contiguous(), kc, vc


def _ratios(case, out):
    inp = inputs(case)
    return check_outputs(*out, case_reference(case), inp.pos, inp.slots)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fp32_emulation_stays_inside_the_bound(case):
    ratios = _ratios(case, emulate(case))
    print("EMU", case.name, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("mut", list(MUTATIONS))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_one_line_slips_leave_the_bound(case, mut):
    ratios = _ratios(case, emulate(case, mut))
    hit = MUTATIONS[mut]
    assert max(ratios[s] for s in hit) > 1.0, ratios
    assert max(r for s, r in ratios.items() if s not in hit) <= 1.0, ratios


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    assert {c.D for c in CASES} == {64, 128} and {c.theta for c in CASES} == {1e4, 1e6}
    for Dd in (64, 128):
        assert {c.H // c.Hkv for c in CASES if c.D == Dd} == {1, 2, 4, 8}
        assert {c.rows for c in CASES if c.D == Dd} == {1, 3, 16, 17, 40, 64}
    seen = set()
    for c in CASES:
        inp = inputs(c)
        pos, slots = inp.pos.tolist(), inp.slots.tolist()
        seen |= {"first" if p == 0 else "last" if p == c.max_seq - 1 else "middle" for p in pos}
        assert len(set(zip(slots, pos))) == c.rows and max(slots) < c.n_slots and 4 not in slots
        if c.rows > 11:
            chunk = [p for p, s in zip(pos, slots) if s == 2]
            assert chunk == list(range(chunk[0], chunk[0] + 8)) and slots.count(c.n_slots - 1) == c.rows - 11
        heads = inp.qkv.view(c.rows, -1, c.D).float()
        ms = heads[:, :c.H + c.Hkv].pow(2).mean(-1)
        assert bool((ms == 0).any()) and bool((ms > 2.0 ** 70).any())
        assert c.rows == 1 or bool(((ms > 0) & (ms < EPS)).any())  # eps-dominated, but not zero
    assert seen == {"first", "middle", "last"}
    assert any(c.no_slots for c in CASES)


# ---------------------------------------------------------------- the engine test's prompts (see test_gpu_qk_norm)
def test_engine_prompts_are_confident():
    # The greedy continuations the GPU test expects, from the fp32 reference, each with a top-2 gap of at least
    # 3 % of the largest logit: bf16-level differences between a 1-row step and a 16-row graph cannot flip them.
    from p2p_llm_tunnel_amd.models.tiny_llm import TinyLlama
    m = TinyLlama(QK2, device="cpu", max_batch=1, seed=0)
    for prompt, want in ENGINE_PROMPTS:
        seq = list(prompt)
        for k in range(len(want)):
            lg = m.reference_logits(torch.tensor([seq]))[0]
            top = lg.topk(2).values
            assert float(top[0] - top[1]) >= 0.03 * float(lg.abs().max()), (len(prompt), k)
            assert int(lg.argmax()) == want[k]
            seq.append(want[k])


# ---------------------------------------------------------------- chat_template_kwargs, generation_config.json
THINK_TEMPLATE = ("{{ bos_token }}{% for m in messages %}<|{{ m['role'] }}|>{{ m['content'] }}{{ eos_token }}{% endfor %}"
                  "{% if add_generation_prompt %}<|assistant|>"
                  "{% if enable_thinking is defined and enable_thinking is false %}<think></think>{% endif %}"
                  "{% if tag is defined %}{{ tag }}{% endif %}{% endif %}")


def _thinking_tokenizer(path):
    _tokenizer_dir(str(path))
    (path / "tokenizer_config.json").write_text(json.dumps(
        {"bos_token": "<s>", "eos_token": {"content": "</s>"}, "chat_template": THINK_TEMPLATE}))
    return Tokenizer(str(path))


def test_chat_template_kwargs_reach_the_template(tmp_path):
    from p2p_llm_tunnel_amd.models.server import Engine, _prompt_ids, chat_template_kwargs, start_server
    tok = _thinking_tokenizer(tmp_path)
    msgs = [{"role": "user", "content": "hello world"}]
    text = lambda ids: tok.tok.decode(ids, skip_special_tokens=False)
    base = "<s><|user|>hello world</s><|assistant|>"
    assert text(tok.chat(msgs)) == base == text(tok.chat(msgs, template_kwargs={"enable_thinking": True}))
    assert text(tok.chat(msgs, template_kwargs={"enable_thinking": False})) == base + "<think></think>"
    # the variables the render sets itself cannot be overridden
    assert text(tok.chat(msgs, template_kwargs={"add_generation_prompt": False, "messages": [], "tag": "x"})) == base + "x"
    body = {"messages": msgs, "chat_template_kwargs": {"enable_thinking": False}}
    assert text(_prompt_ids(body, tok, chat_template_kwargs(body))) == base + "<think></think>"
    assert chat_template_kwargs({"messages": msgs}) is None

    eng = Engine(max_batch=4, model=_FakeModel(tok.tok.get_vocab_size()))
    srv, port, _ = start_server(port=0, engine=eng, model_name="ckpt", tokenizer=tok)
    try:
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=20)

        def post(extra):
            c.request("POST", "/v1/chat/completions", body=json.dumps({"stream": False, "max_tokens": 4, "messages": msgs,
                                                                       **extra}))
            r = c.getresponse()
            return r.status, json.loads(r.read())
        plain = post({})
        on = post({"chat_template_kwargs": {"enable_thinking": True}})
        assert plain[0] == 200 == on[0] and _text(on) == _text(plain)
        off = post({"chat_template_kwargs": {"enable_thinking": False, "tag": None}})
        # the fake model's continuation depends on the prompt's last token and length: another prompt, another text
        assert off[0] == 200 and _text(off) != _text(plain)
        for bad in (["enable_thinking"], "enable_thinking=false", 1, True, {"enable_thinking": {"x": 1}},
                    {"enable_thinking": [False]}):
            status, j = post({"chat_template_kwargs": bad})
            assert status == 400 and "chat_template_kwargs" in j["error"]["message"], (bad, j)
        assert post({"chat_template_kwargs": None})[0] == 200
    finally:
        srv.shutdown()
        eng.stop()


def _text(resp):
    return resp[1]["choices"][0]["message"]["content"]


def test_eos_ids_from_generation_config(tmp_path):
    _tokenizer_dir(str(tmp_path))
    conf = {k: v for k, v in CONF.items()}
    (tmp_path / "config.json").write_text(json.dumps(dict(conf, eos_token_id=7)))
    assert Tokenizer.for_checkpoint(str(tmp_path)).eos_ids == {7}
    (tmp_path / "generation_config.json").write_text(json.dumps({"eos_token_id": [7, 9], "temperature": 0.6}))
    assert Tokenizer.for_checkpoint(str(tmp_path)).eos_ids == {7, 9}
    (tmp_path / "generation_config.json").write_text(json.dumps({"eos_token_id": 11}))
    assert Tokenizer.for_checkpoint(str(tmp_path)).eos_ids == {7, 11}
    (tmp_path / "config.json").write_text(json.dumps(conf))  # no id in config.json: the list alone
    (tmp_path / "generation_config.json").write_text(json.dumps({"eos_token_id": [3, 5]}))
    assert Tokenizer.for_checkpoint(str(tmp_path)).eos_ids == {3, 5}
    (tmp_path / "generation_config.json").write_text("{not json")  # unreadable: config.json's ids, else the token's
    assert Tokenizer.for_checkpoint(str(tmp_path)).eos_ids == {Tokenizer(str(tmp_path)).tok.token_to_id("</s>")}
