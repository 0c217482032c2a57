"""The fused step's weight table, held to one description (CPU only).

* The wire format did not move: for six model families, each with bf16 and with FP8 weights, the table that
  ``TinyLlama.fused_weights`` builds has the recorded length and, entry by entry, the recorded dtype, shape and
  SHA-256 of its bytes. ``GOLDEN`` was recorded by running ``digests`` below, as it stands, on the commit before
  ``ops.WeightTable`` existed (``python tests/test_weight_table.py`` printed it there); it is never regenerated from
  the code under test. The weights come from integer patterns cast to bf16, no RNG.
* Python and C agree: ``ops.WeightTable`` and the library's own accessor (``p2pt_llama_weight_layout``, which asks
  the struct the step reads its pointers through) give the same length and the same index for every (role, layer).
* The constructor refuses a wrong entry by name, from shapes and dtypes alone, before it needs a device.
"""
import ctypes
import hashlib
import os
import sys
from dataclasses import replace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from p2p_llm_tunnel_amd import ops  # noqa: E402
from p2p_llm_tunnel_amd.models.rope import RopeScaling  # noqa: E402
from p2p_llm_tunnel_amd.models.tiny_llm import LlamaConfig, TinyLlama, llama_dims  # noqa: E402

BF = torch.bfloat16
# The smallest legal shape, two layers.
BASE = LlamaConfig(vocab=64, dim=64, n_layers=2, n_heads=2, n_kv_heads=1, head_dim=64, ffn=64, max_seq=8)
ROPE = RopeScaling("llama3", 8.0, 1.0, 4.0, 64)
FAMILIES = {"plain": {}, "qkv_bias": dict(qkv_bias=True), "qk_norm": dict(qk_norm=True),
            "rope": dict(rope_scaling=ROPE), "rope_qkv_bias": dict(rope_scaling=ROPE, qkv_bias=True),
            "rope_qk_norm": dict(rope_scaling=ROPE, qk_norm=True)}
TIED = ("plain", "rope_qk_norm")  # lm_head is the embedding itself; untied elsewhere
FORMATS = ("bf16", "fp8")
CASES = [(f, w) for f in FAMILIES for w in FORMATS]


def pattern(salt, *shape):
    """Multiples of 1/128 in [-125/128, 125/128] (exact in bf16), a different run for every salt; a row of 64 or 128
    sees only part of the 251 values, so the rows' maxima, and with them their FP8 scales, differ."""
    n = 1
    for s in shape:
        n *= s
    return (((torch.arange(n) * 37 + salt * 11) % 251 - 125).float() / 128).to(BF).view(*shape)


def norm_pattern(salt, n):
    """1 + k / 32, k in -8 .. 8 (exact in bf16), a different run for every salt in 0 .. 16."""
    return (1 + ((torch.arange(n) * 5 + salt) % 17 - 8).float() / 32).to(BF)


def model(family, weight_dtype, n_layers=2):
    c = replace(BASE, n_layers=n_layers, **FAMILIES[family])
    n_qkv = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim
    layers = []
    for i in range(n_layers):
        s = 20 * i
        L = {"attn_norm": norm_pattern(4 * i, c.dim), "wqkv": pattern(s + 2, n_qkv, c.dim),
             "wo": pattern(s + 3, c.dim, c.n_heads * c.head_dim), "ffn_norm": norm_pattern(4 * i + 1, c.dim),
             "w_gate_up": pattern(s + 5, 2 * c.ffn, c.dim), "w_down": pattern(s + 6, c.dim, c.ffn)}
        if c.qk_norm:
            L.update(q_norm=norm_pattern(4 * i + 2, c.head_dim), k_norm=norm_pattern(4 * i + 3, c.head_dim))
        if c.qkv_bias:
            L.update(bqkv=pattern(s + 9, n_qkv))
        layers.append(L)
    embed = pattern(101, c.vocab, c.dim)
    weights = {"embed": embed, "final_norm": norm_pattern(16, c.dim),
               "lm_head": embed if family in TIED else pattern(103, c.vocab, c.dim), "layers": layers}
    return TinyLlama.from_weights(c, weights, device="cpu", max_batch=1, weight_dtype=weight_dtype)


def digests(table):
    """One line per entry: dtype, shape, SHA-256 of the bytes."""
    out = []
    for t in table:
        raw = t.contiguous().view(torch.uint8).numpy().tobytes()
        out.append(f"{str(t.dtype)[6:]} {'x'.join(map(str, t.shape))} {hashlib.sha256(raw).hexdigest()}")
    return out


# Recorded on the parent commit (module docstring). Never regenerate these from the code under test.
GOLDEN = {
    ('plain', 'bf16'): [
        'bfloat16 64x64 bd205fdca6be621afafc6b0af233acbc1c4e45a08cd55366c8ab4a9e09195493',
        'bfloat16 64 0a3a8376025c9def582b5585f94594420da7cbd700ffb31ddf041cfcd3b9acd1',
        'bfloat16 64x64 6771f2a2c4aaccb068d7687da53a90f1b334863270b6aec139a8417683d62a02',
        'bfloat16 64 53de521d5d847bb42a1ee2110ac6a86e57ffba29e99bfa029b56c342d5be51f3',
        'bfloat16 256x64 b2e634bb79b4e1550dc2f745cc75577bfeb56582c8cf62ad3b0753baa238c77d',
        'bfloat16 64x128 1d9d037d1d78806abda276f129b04b95c648c920c0995440286f0b4ea82ee609',
        'bfloat16 64 e7396f9dea72a73b4dbd63a7537a4e8d36324b92cf4d6c22d18563e544779d80',
        'bfloat16 128x64 d93a06ddb73452c7a0c37387ef835e7b0ea7a8c07f67d1b080edf604d1075fa3',
        'bfloat16 64x64 d95e315b4c0b64dee0ba324eedf80b83074ad810e204d393ffcfdace9a6ee065',
        'bfloat16 64 638e336c111cd12a642fa16522befc99f89350c1cea3a0cd72c4d2e9b1f94cf4',
        'bfloat16 256x64 22c59d26eb21bfe4b75e6f4f94cfd4ef08a9732b284523f9140a9e549d73e866',
        'bfloat16 64x128 d6531f1d297073c712818832ee64ff0c0510eb1489c687869f41a2c68d908dfc',
        'bfloat16 64 bbf879e4cd1923f562418063cf896b86608b07437dd211b1e1d0e357c072ae84',
        'bfloat16 128x64 32c877abe9d2fcc549a43dfb93a9e22d4cc0ac8dcde09b6382557c5f7a260c54',
        'bfloat16 64x64 ca4864a77b93f03b75bf820c584371871f4691c60ef0607c53d1da21c14c9c7b',
    ],
    ('plain', 'fp8'): [
        'bfloat16 64x64 bd205fdca6be621afafc6b0af233acbc1c4e45a08cd55366c8ab4a9e09195493',
        'bfloat16 64 0a3a8376025c9def582b5585f94594420da7cbd700ffb31ddf041cfcd3b9acd1',
        'float8_e4m3fn 64x64 fbf69f311ae1a0a4932a03418ae22d658ed8cefc50f90759a0cb86af8c9f66d4',
        'bfloat16 64 53de521d5d847bb42a1ee2110ac6a86e57ffba29e99bfa029b56c342d5be51f3',
        'float8_e4m3fn 256x64 c34beeb805106cc5186d4fe786e05941422a369a6647aacce5a5cc83b8d2196a',
        'float8_e4m3fn 64x128 ab63212237abc5c45d3d09c277edb64c9816bfcf9ea54fc6caf35fa2e01948b6',
        'bfloat16 64 e7396f9dea72a73b4dbd63a7537a4e8d36324b92cf4d6c22d18563e544779d80',
        'float8_e4m3fn 128x64 52bef89076f88d4d489f1b4f93818f3a46d312cd7e261423d3e2dbfe9d6f7e58',
        'float8_e4m3fn 64x64 d8e37bae03c2223f4c8096756d2f485869c6cadfa3ef0ecd3638779d5b18eb1e',
        'bfloat16 64 638e336c111cd12a642fa16522befc99f89350c1cea3a0cd72c4d2e9b1f94cf4',
        'float8_e4m3fn 256x64 ab261b9c04ef7e452b5afc2033d73e66ecb5ac25992d396152c72751defd527a',
        'float8_e4m3fn 64x128 3d230576643c35ebded117cd207eb7b5049a6b8b79af4ebd992378cea5b04caa',
        'bfloat16 64 bbf879e4cd1923f562418063cf896b86608b07437dd211b1e1d0e357c072ae84',
        'float8_e4m3fn 128x64 2e2658a95cb52cc35affd78ba1f91f1fad70a497f75751bd69a4fbe972616807',
        'float8_e4m3fn 64x64 f6b43e1ac0ff19f9fa251d61ffbddf3e2794fd297eeee68c8f6163e684845a55',
        'float32 64 8ef5fa9c8270c277116ffe6efec7b20e0eb3b3f4881e76e8a633d5a7ee37a736',
        'float32 256 56f1cb3d17cec094f66868412a8983df0b8ffdeba49ea09224e2151eb149b4b2',
        'float32 64 1a63ebb7cb488b8298d92d61875b750802cdd1cc29cb08ccdf25f6d2132bacd4',
        'float32 128 252067e87983f627cca3d00d67416c8c3b7bf3addb84dd2b33473b053e780c2c',
        'float32 64 ac093d85dfe2b4e166199996aeb62f8ceebeaa82d27331ca6b1d01b274a7bda6',
        'float32 256 8fe55e92302d42d9bda06eca7faadd95050c4b6bd45fb4348b6a6e4fab777758',
        'float32 64 36605685a934da837938a0102cc7d44752917903c318600bea46ff7dedca2eac',
        'float32 128 04ba6e611328741cab16d719318910a3a0611251a696fb398e406869745256c1',
        'float32 64 944f9d05dac705257acbd8c044183c2c107cc4bc2f7b09b632027a78a1e604e7',
    ],
    ('qkv_bias', 'bf16'): [
        'bfloat16 64x64 bd205fdca6be621afafc6b0af233acbc1c4e45a08cd55366c8ab4a9e09195493',
        'bfloat16 64 0a3a8376025c9def582b5585f94594420da7cbd700ffb31ddf041cfcd3b9acd1',
        'bfloat16 64x64 2d67da4b7370ce39ad387757ec3ae9ff99d6e18884cc39459b6df0ac0e1730fa',
        'bfloat16 64 53de521d5d847bb42a1ee2110ac6a86e57ffba29e99bfa029b56c342d5be51f3',
        'bfloat16 256x64 b2e634bb79b4e1550dc2f745cc75577bfeb56582c8cf62ad3b0753baa238c77d',
        'bfloat16 64x128 1d9d037d1d78806abda276f129b04b95c648c920c0995440286f0b4ea82ee609',
        'bfloat16 64 e7396f9dea72a73b4dbd63a7537a4e8d36324b92cf4d6c22d18563e544779d80',
        'bfloat16 128x64 d93a06ddb73452c7a0c37387ef835e7b0ea7a8c07f67d1b080edf604d1075fa3',
        'bfloat16 64x64 d95e315b4c0b64dee0ba324eedf80b83074ad810e204d393ffcfdace9a6ee065',
        'bfloat16 256 4b4c5fd6617b29a7653fb2dfb1eba6fae67a4aa0069854070586e1aca9790e3b',
        'bfloat16 64 638e336c111cd12a642fa16522befc99f89350c1cea3a0cd72c4d2e9b1f94cf4',
        'bfloat16 256x64 22c59d26eb21bfe4b75e6f4f94cfd4ef08a9732b284523f9140a9e549d73e866',
        'bfloat16 64x128 d6531f1d297073c712818832ee64ff0c0510eb1489c687869f41a2c68d908dfc',
        'bfloat16 64 bbf879e4cd1923f562418063cf896b86608b07437dd211b1e1d0e357c072ae84',
        'bfloat16 128x64 32c877abe9d2fcc549a43dfb93a9e22d4cc0ac8dcde09b6382557c5f7a260c54',
        'bfloat16 64x64 ca4864a77b93f03b75bf820c584371871f4691c60ef0607c53d1da21c14c9c7b',
        'bfloat16 256 9d383ced035f146daf6336be1522b6d7d52f49697467e2f17f13edb63f92dd35',
    ],
    ('qkv_bias', 'fp8'): [
        'bfloat16 64x64 bd205fdca6be621afafc6b0af233acbc1c4e45a08cd55366c8ab4a9e09195493',
        'bfloat16 64 0a3a8376025c9def582b5585f94594420da7cbd700ffb31ddf041cfcd3b9acd1',
        'float8_e4m3fn 64x64 260d47940e6e216173e0bdeca51771d5a6e3a4940e1e21817ee0f85ab460c122',
        'bfloat16 64 53de521d5d847bb42a1ee2110ac6a86e57ffba29e99bfa029b56c342d5be51f3',
        'float8_e4m3fn 256x64 c34beeb805106cc5186d4fe786e05941422a369a6647aacce5a5cc83b8d2196a',
        'float8_e4m3fn 64x128 ab63212237abc5c45d3d09c277edb64c9816bfcf9ea54fc6caf35fa2e01948b6',
        'bfloat16 64 e7396f9dea72a73b4dbd63a7537a4e8d36324b92cf4d6c22d18563e544779d80',
        'float8_e4m3fn 128x64 52bef89076f88d4d489f1b4f93818f3a46d312cd7e261423d3e2dbfe9d6f7e58',
        'float8_e4m3fn 64x64 d8e37bae03c2223f4c8096756d2f485869c6cadfa3ef0ecd3638779d5b18eb1e',
        'bfloat16 256 4b4c5fd6617b29a7653fb2dfb1eba6fae67a4aa0069854070586e1aca9790e3b',
        'bfloat16 64 638e336c111cd12a642fa16522befc99f89350c1cea3a0cd72c4d2e9b1f94cf4',
        'float8_e4m3fn 256x64 ab261b9c04ef7e452b5afc2033d73e66ecb5ac25992d396152c72751defd527a',
        'float8_e4m3fn 64x128 3d230576643c35ebded117cd207eb7b5049a6b8b79af4ebd992378cea5b04caa',
        'bfloat16 64 bbf879e4cd1923f562418063cf896b86608b07437dd211b1e1d0e357c072ae84',
        'float8_e4m3fn 128x64 2e2658a95cb52cc35affd78ba1f91f1fad70a497f75751bd69a4fbe972616807',
        'float8_e4m3fn 64x64 f6b43e1ac0ff19f9fa251d61ffbddf3e2794fd297eeee68c8f6163e684845a55',
        'bfloat16 256 9d383ced035f146daf6336be1522b6d7d52f49697467e2f17f13edb63f92dd35',
        'float32 64 13ab2ca7b1c380998c3ac71dae95fe307f32632354b4cd37791e42415f6b5424',
        'float32 256 56f1cb3d17cec094f66868412a8983df0b8ffdeba49ea09224e2151eb149b4b2',
        'float32 64 1a63ebb7cb488b8298d92d61875b750802cdd1cc29cb08ccdf25f6d2132bacd4',
        'float32 128 252067e87983f627cca3d00d67416c8c3b7bf3addb84dd2b33473b053e780c2c',
        'float32 64 ac093d85dfe2b4e166199996aeb62f8ceebeaa82d27331ca6b1d01b274a7bda6',
        'float32 256 8fe55e92302d42d9bda06eca7faadd95050c4b6bd45fb4348b6a6e4fab777758',
        'float32 64 36605685a934da837938a0102cc7d44752917903c318600bea46ff7dedca2eac',
        'float32 128 04ba6e611328741cab16d719318910a3a0611251a696fb398e406869745256c1',
        'float32 64 944f9d05dac705257acbd8c044183c2c107cc4bc2f7b09b632027a78a1e604e7',
    ],
    ('qk_norm', 'bf16'): [
        'bfloat16 64x64 bd205fdca6be621afafc6b0af233acbc1c4e45a08cd55366c8ab4a9e09195493',
        'bfloat16 64 0a3a8376025c9def582b5585f94594420da7cbd700ffb31ddf041cfcd3b9acd1',
        'bfloat16 64x64 2d67da4b7370ce39ad387757ec3ae9ff99d6e18884cc39459b6df0ac0e1730fa',
        'bfloat16 64 53de521d5d847bb42a1ee2110ac6a86e57ffba29e99bfa029b56c342d5be51f3',
        'bfloat16 256x64 43666e069fb17c1ff2d3586f65f1c867c9c7188f37672b7c12c9d0abb50bdd21',
        'bfloat16 64x128 1d9d037d1d78806abda276f129b04b95c648c920c0995440286f0b4ea82ee609',
        'bfloat16 64 e7396f9dea72a73b4dbd63a7537a4e8d36324b92cf4d6c22d18563e544779d80',
        'bfloat16 128x64 d93a06ddb73452c7a0c37387ef835e7b0ea7a8c07f67d1b080edf604d1075fa3',
        'bfloat16 64x64 d95e315b4c0b64dee0ba324eedf80b83074ad810e204d393ffcfdace9a6ee065',
        'bfloat16 64 042ad6b65c6259905f314368de4d180ab4595f6e2a2d0cc4669c934d0f2c3a75',
        'bfloat16 64 93470d3c0c02e42d35789d38e133c0eb8b20a6191543f4db4f3f04b144b6c521',
        'bfloat16 64 638e336c111cd12a642fa16522befc99f89350c1cea3a0cd72c4d2e9b1f94cf4',
        'bfloat16 256x64 d7d803a8caa975f50d9f729ceefbaf3ea499f90cc2878db1297fbdab7f88b498',
        'bfloat16 64x128 d6531f1d297073c712818832ee64ff0c0510eb1489c687869f41a2c68d908dfc',
        'bfloat16 64 bbf879e4cd1923f562418063cf896b86608b07437dd211b1e1d0e357c072ae84',
        'bfloat16 128x64 32c877abe9d2fcc549a43dfb93a9e22d4cc0ac8dcde09b6382557c5f7a260c54',
        'bfloat16 64x64 ca4864a77b93f03b75bf820c584371871f4691c60ef0607c53d1da21c14c9c7b',
        'bfloat16 64 a7371f6fbce9f49fc62e2e94aaa869a5f079fd33f7d65ed1117f61b638f28b4b',
        'bfloat16 64 fac48e7c89b1a00dfc352d71a0b7ec4828f2329353fb4903085c0bf99f0136e1',
    ],
    ('qk_norm', 'fp8'): [
        'bfloat16 64x64 bd205fdca6be621afafc6b0af233acbc1c4e45a08cd55366c8ab4a9e09195493',
        'bfloat16 64 0a3a8376025c9def582b5585f94594420da7cbd700ffb31ddf041cfcd3b9acd1',
        'float8_e4m3fn 64x64 260d47940e6e216173e0bdeca51771d5a6e3a4940e1e21817ee0f85ab460c122',
        'bfloat16 64 53de521d5d847bb42a1ee2110ac6a86e57ffba29e99bfa029b56c342d5be51f3',
        'float8_e4m3fn 256x64 9fe3fd26ec0bf452587db2b20a8bbb8cd80ddcb2e23a27a8f2ab654448916b9e',
        'float8_e4m3fn 64x128 ab63212237abc5c45d3d09c277edb64c9816bfcf9ea54fc6caf35fa2e01948b6',
        'bfloat16 64 e7396f9dea72a73b4dbd63a7537a4e8d36324b92cf4d6c22d18563e544779d80',
        'float8_e4m3fn 128x64 52bef89076f88d4d489f1b4f93818f3a46d312cd7e261423d3e2dbfe9d6f7e58',
        'float8_e4m3fn 64x64 d8e37bae03c2223f4c8096756d2f485869c6cadfa3ef0ecd3638779d5b18eb1e',
        'bfloat16 64 042ad6b65c6259905f314368de4d180ab4595f6e2a2d0cc4669c934d0f2c3a75',
        'bfloat16 64 93470d3c0c02e42d35789d38e133c0eb8b20a6191543f4db4f3f04b144b6c521',
        'bfloat16 64 638e336c111cd12a642fa16522befc99f89350c1cea3a0cd72c4d2e9b1f94cf4',
        'float8_e4m3fn 256x64 05dc907334824afbb14ce4d4a502479b0711f94780e2958b6b1bbed9411e132b',
        'float8_e4m3fn 64x128 3d230576643c35ebded117cd207eb7b5049a6b8b79af4ebd992378cea5b04caa',
        'bfloat16 64 bbf879e4cd1923f562418063cf896b86608b07437dd211b1e1d0e357c072ae84',
        'float8_e4m3fn 128x64 2e2658a95cb52cc35affd78ba1f91f1fad70a497f75751bd69a4fbe972616807',
        'float8_e4m3fn 64x64 f6b43e1ac0ff19f9fa251d61ffbddf3e2794fd297eeee68c8f6163e684845a55',
        'bfloat16 64 a7371f6fbce9f49fc62e2e94aaa869a5f079fd33f7d65ed1117f61b638f28b4b',
        'bfloat16 64 fac48e7c89b1a00dfc352d71a0b7ec4828f2329353fb4903085c0bf99f0136e1',
        'float32 64 13ab2ca7b1c380998c3ac71dae95fe307f32632354b4cd37791e42415f6b5424',
        'float32 256 16fc0e7b2ce4a32bfaa0c7f8de7bcdcb57bdcf4dd56a947e0050d685a825c75f',
        'float32 64 1a63ebb7cb488b8298d92d61875b750802cdd1cc29cb08ccdf25f6d2132bacd4',
        'float32 128 252067e87983f627cca3d00d67416c8c3b7bf3addb84dd2b33473b053e780c2c',
        'float32 64 ac093d85dfe2b4e166199996aeb62f8ceebeaa82d27331ca6b1d01b274a7bda6',
        'float32 256 ea1b7620b87ea31732e4f593c2c96fce12cbb3132b8be27a41ffe19066b94687',
        'float32 64 36605685a934da837938a0102cc7d44752917903c318600bea46ff7dedca2eac',
        'float32 128 04ba6e611328741cab16d719318910a3a0611251a696fb398e406869745256c1',
        'float32 64 944f9d05dac705257acbd8c044183c2c107cc4bc2f7b09b632027a78a1e604e7',
    ],
    ('rope', 'bf16'): [
        'bfloat16 64x64 bd205fdca6be621afafc6b0af233acbc1c4e45a08cd55366c8ab4a9e09195493',
        'bfloat16 64 0a3a8376025c9def582b5585f94594420da7cbd700ffb31ddf041cfcd3b9acd1',
        'bfloat16 64x64 2d67da4b7370ce39ad387757ec3ae9ff99d6e18884cc39459b6df0ac0e1730fa',
        'float32 32 ee3f5bc867a3e580ce257e9aafb9b234c4bd580a081d321138c8058166a3865d',
        'bfloat16 64 53de521d5d847bb42a1ee2110ac6a86e57ffba29e99bfa029b56c342d5be51f3',
        'bfloat16 256x64 b2e634bb79b4e1550dc2f745cc75577bfeb56582c8cf62ad3b0753baa238c77d',
        'bfloat16 64x128 1d9d037d1d78806abda276f129b04b95c648c920c0995440286f0b4ea82ee609',
        'bfloat16 64 e7396f9dea72a73b4dbd63a7537a4e8d36324b92cf4d6c22d18563e544779d80',
        'bfloat16 128x64 d93a06ddb73452c7a0c37387ef835e7b0ea7a8c07f67d1b080edf604d1075fa3',
        'bfloat16 64x64 d95e315b4c0b64dee0ba324eedf80b83074ad810e204d393ffcfdace9a6ee065',
        'bfloat16 64 638e336c111cd12a642fa16522befc99f89350c1cea3a0cd72c4d2e9b1f94cf4',
        'bfloat16 256x64 22c59d26eb21bfe4b75e6f4f94cfd4ef08a9732b284523f9140a9e549d73e866',
        'bfloat16 64x128 d6531f1d297073c712818832ee64ff0c0510eb1489c687869f41a2c68d908dfc',
        'bfloat16 64 bbf879e4cd1923f562418063cf896b86608b07437dd211b1e1d0e357c072ae84',
        'bfloat16 128x64 32c877abe9d2fcc549a43dfb93a9e22d4cc0ac8dcde09b6382557c5f7a260c54',
        'bfloat16 64x64 ca4864a77b93f03b75bf820c584371871f4691c60ef0607c53d1da21c14c9c7b',
    ],
    ('rope', 'fp8'): [
        'bfloat16 64x64 bd205fdca6be621afafc6b0af233acbc1c4e45a08cd55366c8ab4a9e09195493',
        'bfloat16 64 0a3a8376025c9def582b5585f94594420da7cbd700ffb31ddf041cfcd3b9acd1',
        'float8_e4m3fn 64x64 260d47940e6e216173e0bdeca51771d5a6e3a4940e1e21817ee0f85ab460c122',
        'float32 32 ee3f5bc867a3e580ce257e9aafb9b234c4bd580a081d321138c8058166a3865d',
        'bfloat16 64 53de521d5d847bb42a1ee2110ac6a86e57ffba29e99bfa029b56c342d5be51f3',
        'float8_e4m3fn 256x64 c34beeb805106cc5186d4fe786e05941422a369a6647aacce5a5cc83b8d2196a',
        'float8_e4m3fn 64x128 ab63212237abc5c45d3d09c277edb64c9816bfcf9ea54fc6caf35fa2e01948b6',
        'bfloat16 64 e7396f9dea72a73b4dbd63a7537a4e8d36324b92cf4d6c22d18563e544779d80',
        'float8_e4m3fn 128x64 52bef89076f88d4d489f1b4f93818f3a46d312cd7e261423d3e2dbfe9d6f7e58',
        'float8_e4m3fn 64x64 d8e37bae03c2223f4c8096756d2f485869c6cadfa3ef0ecd3638779d5b18eb1e',
        'bfloat16 64 638e336c111cd12a642fa16522befc99f89350c1cea3a0cd72c4d2e9b1f94cf4',
        'float8_e4m3fn 256x64 ab261b9c04ef7e452b5afc2033d73e66ecb5ac25992d396152c72751defd527a',
        'float8_e4m3fn 64x128 3d230576643c35ebded117cd207eb7b5049a6b8b79af4ebd992378cea5b04caa',
        'bfloat16 64 bbf879e4cd1923f562418063cf896b86608b07437dd211b1e1d0e357c072ae84',
        'float8_e4m3fn 128x64 2e2658a95cb52cc35affd78ba1f91f1fad70a497f75751bd69a4fbe972616807',
        'float8_e4m3fn 64x64 f6b43e1ac0ff19f9fa251d61ffbddf3e2794fd297eeee68c8f6163e684845a55',
        'float32 64 13ab2ca7b1c380998c3ac71dae95fe307f32632354b4cd37791e42415f6b5424',
        'float32 256 56f1cb3d17cec094f66868412a8983df0b8ffdeba49ea09224e2151eb149b4b2',
        'float32 64 1a63ebb7cb488b8298d92d61875b750802cdd1cc29cb08ccdf25f6d2132bacd4',
        'float32 128 252067e87983f627cca3d00d67416c8c3b7bf3addb84dd2b33473b053e780c2c',
        'float32 64 ac093d85dfe2b4e166199996aeb62f8ceebeaa82d27331ca6b1d01b274a7bda6',
        'float32 256 8fe55e92302d42d9bda06eca7faadd95050c4b6bd45fb4348b6a6e4fab777758',
        'float32 64 36605685a934da837938a0102cc7d44752917903c318600bea46ff7dedca2eac',
        'float32 128 04ba6e611328741cab16d719318910a3a0611251a696fb398e406869745256c1',
        'float32 64 944f9d05dac705257acbd8c044183c2c107cc4bc2f7b09b632027a78a1e604e7',
    ],
    ('rope_qkv_bias', 'bf16'): [
        'bfloat16 64x64 bd205fdca6be621afafc6b0af233acbc1c4e45a08cd55366c8ab4a9e09195493',
        'bfloat16 64 0a3a8376025c9def582b5585f94594420da7cbd700ffb31ddf041cfcd3b9acd1',
        'bfloat16 64x64 2d67da4b7370ce39ad387757ec3ae9ff99d6e18884cc39459b6df0ac0e1730fa',
        'float32 32 ee3f5bc867a3e580ce257e9aafb9b234c4bd580a081d321138c8058166a3865d',
        'bfloat16 64 53de521d5d847bb42a1ee2110ac6a86e57ffba29e99bfa029b56c342d5be51f3',
        'bfloat16 256x64 b2e634bb79b4e1550dc2f745cc75577bfeb56582c8cf62ad3b0753baa238c77d',
        'bfloat16 64x128 1d9d037d1d78806abda276f129b04b95c648c920c0995440286f0b4ea82ee609',
        'bfloat16 64 e7396f9dea72a73b4dbd63a7537a4e8d36324b92cf4d6c22d18563e544779d80',
        'bfloat16 128x64 d93a06ddb73452c7a0c37387ef835e7b0ea7a8c07f67d1b080edf604d1075fa3',
        'bfloat16 64x64 d95e315b4c0b64dee0ba324eedf80b83074ad810e204d393ffcfdace9a6ee065',
        'bfloat16 256 4b4c5fd6617b29a7653fb2dfb1eba6fae67a4aa0069854070586e1aca9790e3b',
        'bfloat16 64 638e336c111cd12a642fa16522befc99f89350c1cea3a0cd72c4d2e9b1f94cf4',
        'bfloat16 256x64 22c59d26eb21bfe4b75e6f4f94cfd4ef08a9732b284523f9140a9e549d73e866',
        'bfloat16 64x128 d6531f1d297073c712818832ee64ff0c0510eb1489c687869f41a2c68d908dfc',
        'bfloat16 64 bbf879e4cd1923f562418063cf896b86608b07437dd211b1e1d0e357c072ae84',
        'bfloat16 128x64 32c877abe9d2fcc549a43dfb93a9e22d4cc0ac8dcde09b6382557c5f7a260c54',
        'bfloat16 64x64 ca4864a77b93f03b75bf820c584371871f4691c60ef0607c53d1da21c14c9c7b',
        'bfloat16 256 9d383ced035f146daf6336be1522b6d7d52f49697467e2f17f13edb63f92dd35',
    ],
    ('rope_qkv_bias', 'fp8'): [
        'bfloat16 64x64 bd205fdca6be621afafc6b0af233acbc1c4e45a08cd55366c8ab4a9e09195493',
        'bfloat16 64 0a3a8376025c9def582b5585f94594420da7cbd700ffb31ddf041cfcd3b9acd1',
        'float8_e4m3fn 64x64 260d47940e6e216173e0bdeca51771d5a6e3a4940e1e21817ee0f85ab460c122',
        'float32 32 ee3f5bc867a3e580ce257e9aafb9b234c4bd580a081d321138c8058166a3865d',
        'bfloat16 64 53de521d5d847bb42a1ee2110ac6a86e57ffba29e99bfa029b56c342d5be51f3',
        'float8_e4m3fn 256x64 c34beeb805106cc5186d4fe786e05941422a369a6647aacce5a5cc83b8d2196a',
        'float8_e4m3fn 64x128 ab63212237abc5c45d3d09c277edb64c9816bfcf9ea54fc6caf35fa2e01948b6',
        'bfloat16 64 e7396f9dea72a73b4dbd63a7537a4e8d36324b92cf4d6c22d18563e544779d80',
        'float8_e4m3fn 128x64 52bef89076f88d4d489f1b4f93818f3a46d312cd7e261423d3e2dbfe9d6f7e58',
        'float8_e4m3fn 64x64 d8e37bae03c2223f4c8096756d2f485869c6cadfa3ef0ecd3638779d5b18eb1e',
        'bfloat16 256 4b4c5fd6617b29a7653fb2dfb1eba6fae67a4aa0069854070586e1aca9790e3b',
        'bfloat16 64 638e336c111cd12a642fa16522befc99f89350c1cea3a0cd72c4d2e9b1f94cf4',
        'float8_e4m3fn 256x64 ab261b9c04ef7e452b5afc2033d73e66ecb5ac25992d396152c72751defd527a',
        'float8_e4m3fn 64x128 3d230576643c35ebded117cd207eb7b5049a6b8b79af4ebd992378cea5b04caa',
        'bfloat16 64 bbf879e4cd1923f562418063cf896b86608b07437dd211b1e1d0e357c072ae84',
        'float8_e4m3fn 128x64 2e2658a95cb52cc35affd78ba1f91f1fad70a497f75751bd69a4fbe972616807',
        'float8_e4m3fn 64x64 f6b43e1ac0ff19f9fa251d61ffbddf3e2794fd297eeee68c8f6163e684845a55',
        'bfloat16 256 9d383ced035f146daf6336be1522b6d7d52f49697467e2f17f13edb63f92dd35',
        'float32 64 13ab2ca7b1c380998c3ac71dae95fe307f32632354b4cd37791e42415f6b5424',
        'float32 256 56f1cb3d17cec094f66868412a8983df0b8ffdeba49ea09224e2151eb149b4b2',
        'float32 64 1a63ebb7cb488b8298d92d61875b750802cdd1cc29cb08ccdf25f6d2132bacd4',
        'float32 128 252067e87983f627cca3d00d67416c8c3b7bf3addb84dd2b33473b053e780c2c',
        'float32 64 ac093d85dfe2b4e166199996aeb62f8ceebeaa82d27331ca6b1d01b274a7bda6',
        'float32 256 8fe55e92302d42d9bda06eca7faadd95050c4b6bd45fb4348b6a6e4fab777758',
        'float32 64 36605685a934da837938a0102cc7d44752917903c318600bea46ff7dedca2eac',
        'float32 128 04ba6e611328741cab16d719318910a3a0611251a696fb398e406869745256c1',
        'float32 64 944f9d05dac705257acbd8c044183c2c107cc4bc2f7b09b632027a78a1e604e7',
    ],
    ('rope_qk_norm', 'bf16'): [
        'bfloat16 64x64 bd205fdca6be621afafc6b0af233acbc1c4e45a08cd55366c8ab4a9e09195493',
        'bfloat16 64 0a3a8376025c9def582b5585f94594420da7cbd700ffb31ddf041cfcd3b9acd1',
        'bfloat16 64x64 6771f2a2c4aaccb068d7687da53a90f1b334863270b6aec139a8417683d62a02',
        'float32 32 ee3f5bc867a3e580ce257e9aafb9b234c4bd580a081d321138c8058166a3865d',
        'bfloat16 64 53de521d5d847bb42a1ee2110ac6a86e57ffba29e99bfa029b56c342d5be51f3',
        'bfloat16 256x64 43666e069fb17c1ff2d3586f65f1c867c9c7188f37672b7c12c9d0abb50bdd21',
        'bfloat16 64x128 1d9d037d1d78806abda276f129b04b95c648c920c0995440286f0b4ea82ee609',
        'bfloat16 64 e7396f9dea72a73b4dbd63a7537a4e8d36324b92cf4d6c22d18563e544779d80',
        'bfloat16 128x64 d93a06ddb73452c7a0c37387ef835e7b0ea7a8c07f67d1b080edf604d1075fa3',
        'bfloat16 64x64 d95e315b4c0b64dee0ba324eedf80b83074ad810e204d393ffcfdace9a6ee065',
        'bfloat16 64 042ad6b65c6259905f314368de4d180ab4595f6e2a2d0cc4669c934d0f2c3a75',
        'bfloat16 64 93470d3c0c02e42d35789d38e133c0eb8b20a6191543f4db4f3f04b144b6c521',
        'bfloat16 64 638e336c111cd12a642fa16522befc99f89350c1cea3a0cd72c4d2e9b1f94cf4',
        'bfloat16 256x64 d7d803a8caa975f50d9f729ceefbaf3ea499f90cc2878db1297fbdab7f88b498',
        'bfloat16 64x128 d6531f1d297073c712818832ee64ff0c0510eb1489c687869f41a2c68d908dfc',
        'bfloat16 64 bbf879e4cd1923f562418063cf896b86608b07437dd211b1e1d0e357c072ae84',
        'bfloat16 128x64 32c877abe9d2fcc549a43dfb93a9e22d4cc0ac8dcde09b6382557c5f7a260c54',
        'bfloat16 64x64 ca4864a77b93f03b75bf820c584371871f4691c60ef0607c53d1da21c14c9c7b',
        'bfloat16 64 a7371f6fbce9f49fc62e2e94aaa869a5f079fd33f7d65ed1117f61b638f28b4b',
        'bfloat16 64 fac48e7c89b1a00dfc352d71a0b7ec4828f2329353fb4903085c0bf99f0136e1',
    ],
    ('rope_qk_norm', 'fp8'): [
        'bfloat16 64x64 bd205fdca6be621afafc6b0af233acbc1c4e45a08cd55366c8ab4a9e09195493',
        'bfloat16 64 0a3a8376025c9def582b5585f94594420da7cbd700ffb31ddf041cfcd3b9acd1',
        'float8_e4m3fn 64x64 fbf69f311ae1a0a4932a03418ae22d658ed8cefc50f90759a0cb86af8c9f66d4',
        'float32 32 ee3f5bc867a3e580ce257e9aafb9b234c4bd580a081d321138c8058166a3865d',
        'bfloat16 64 53de521d5d847bb42a1ee2110ac6a86e57ffba29e99bfa029b56c342d5be51f3',
        'float8_e4m3fn 256x64 9fe3fd26ec0bf452587db2b20a8bbb8cd80ddcb2e23a27a8f2ab654448916b9e',
        'float8_e4m3fn 64x128 ab63212237abc5c45d3d09c277edb64c9816bfcf9ea54fc6caf35fa2e01948b6',
        'bfloat16 64 e7396f9dea72a73b4dbd63a7537a4e8d36324b92cf4d6c22d18563e544779d80',
        'float8_e4m3fn 128x64 52bef89076f88d4d489f1b4f93818f3a46d312cd7e261423d3e2dbfe9d6f7e58',
        'float8_e4m3fn 64x64 d8e37bae03c2223f4c8096756d2f485869c6cadfa3ef0ecd3638779d5b18eb1e',
        'bfloat16 64 042ad6b65c6259905f314368de4d180ab4595f6e2a2d0cc4669c934d0f2c3a75',
        'bfloat16 64 93470d3c0c02e42d35789d38e133c0eb8b20a6191543f4db4f3f04b144b6c521',
        'bfloat16 64 638e336c111cd12a642fa16522befc99f89350c1cea3a0cd72c4d2e9b1f94cf4',
        'float8_e4m3fn 256x64 05dc907334824afbb14ce4d4a502479b0711f94780e2958b6b1bbed9411e132b',
        'float8_e4m3fn 64x128 3d230576643c35ebded117cd207eb7b5049a6b8b79af4ebd992378cea5b04caa',
        'bfloat16 64 bbf879e4cd1923f562418063cf896b86608b07437dd211b1e1d0e357c072ae84',
        'float8_e4m3fn 128x64 2e2658a95cb52cc35affd78ba1f91f1fad70a497f75751bd69a4fbe972616807',
        'float8_e4m3fn 64x64 f6b43e1ac0ff19f9fa251d61ffbddf3e2794fd297eeee68c8f6163e684845a55',
        'bfloat16 64 a7371f6fbce9f49fc62e2e94aaa869a5f079fd33f7d65ed1117f61b638f28b4b',
        'bfloat16 64 fac48e7c89b1a00dfc352d71a0b7ec4828f2329353fb4903085c0bf99f0136e1',
        'float32 64 8ef5fa9c8270c277116ffe6efec7b20e0eb3b3f4881e76e8a633d5a7ee37a736',
        'float32 256 16fc0e7b2ce4a32bfaa0c7f8de7bcdcb57bdcf4dd56a947e0050d685a825c75f',
        'float32 64 1a63ebb7cb488b8298d92d61875b750802cdd1cc29cb08ccdf25f6d2132bacd4',
        'float32 128 252067e87983f627cca3d00d67416c8c3b7bf3addb84dd2b33473b053e780c2c',
        'float32 64 ac093d85dfe2b4e166199996aeb62f8ceebeaa82d27331ca6b1d01b274a7bda6',
        'float32 256 ea1b7620b87ea31732e4f593c2c96fce12cbb3132b8be27a41ffe19066b94687',
        'float32 64 36605685a934da837938a0102cc7d44752917903c318600bea46ff7dedca2eac',
        'float32 128 04ba6e611328741cab16d719318910a3a0611251a696fb398e406869745256c1',
        'float32 64 944f9d05dac705257acbd8c044183c2c107cc4bc2f7b09b632027a78a1e604e7',
    ],
}



# ---------------------------------------------------------------- the wire format did not move
@pytest.mark.parametrize("family,weight_dtype", CASES, ids=[f"{f}-{w}" for f, w in CASES])
def test_the_table_is_the_recorded_one_entry_by_entry(family, weight_dtype):
    m = model(family, weight_dtype)
    table, want = m.fused_weights(), GOLDEN[family, weight_dtype]
    layout = ops.WeightTable(m.dims(), weight_dtype == "fp8")
    assert len(table) == len(want) == len(layout)
    for i, (got, line, e) in enumerate(zip(digests(table), want, layout)):
        assert got == line, (i, e.name, e.layer)
        assert table[i].dtype in e.dtypes and tuple(table[i].shape) == e.shape, (i, e.name, e.layer)


def test_the_recorded_lengths_are_the_wire_format():
    for (family, weight_dtype), want in GOLDEN.items():
        f = FAMILIES[family]
        per = 8 if f.get("qk_norm") else 7 if f.get("qkv_bias") else 6
        assert len(want) == 3 + ("rope_scaling" in f) + per * 2 + (1 + 4 * 2 if weight_dtype == "fp8" else 0)
    assert {f for f in TIED} < set(FAMILIES) and set(FAMILIES) - set(TIED)  # tied and untied, once each at least


def test_lookups_refuse_an_absent_role():
    plain = ops.WeightTable(model("plain", "bf16").dims())
    assert plain.index("lm_head") == 2 and plain.index("wqkv", 1) == 3 + 6 + 1
    for name, layer in (("bqkv", 0), ("q_norm", 1), ("inv_freq", None), ("wqkv", 2), ("wqkv", None), ("embed", 0)):
        with pytest.raises(KeyError, match=name):
            plain.index(name, layer)
    with pytest.raises(KeyError, match="scale"):
        plain.scale_index("w_down", 0)
    f8 = ops.WeightTable(model("rope_qkv_bias", "fp8").dims(), True)
    assert f8.index("inv_freq") == 3 and f8.index("bqkv", 1) == 4 + 7 + 6
    assert f8.scale_index("lm_head") == 4 + 14 and f8.scale_index("w_down", 1) == len(f8) - 1
    with pytest.raises(KeyError, match="attn_norm scale"):
        f8.scale_index("attn_norm", 0)


# ---------------------------------------------------------------- Python and C agree
# decode_fused.hip's enum Role, in its order: what p2pt_llama_weight_layout reports an index for, per layer.
ROLES = ("embed", "final_norm", "lm_head", "inv_freq", "attn_norm", "wqkv", "wo", "ffn_norm", "w_gate_up", "w_down",
         "bqkv", "q_norm", "k_norm")


def _lib_or_skip():
    try:
        return ops.lib()
    except (OSError, RuntimeError) as e:  # no hipcc and no prebuilt library on this host
        pytest.skip(f"the HIP library is not available: {e}")


def library_layout(lib, dims, w8):
    """(return value, index, scale_index) of the library's query, the dicts keyed like ``WeightTable.index``'s
    arguments and holding only what exists."""
    n = len(ROLES) * dims.n_layers
    at, sc, wp = (ctypes.c_int * n)(), (ctypes.c_int * n)(), ops.WeightPlan(w8=w8)
    size = lib.p2pt_llama_weight_layout(ctypes.byref(dims), ctypes.byref(wp), at, sc, n)
    key = lambda j: (ROLES[j % len(ROLES)], None if j % len(ROLES) < 4 else j // len(ROLES))
    # a global role is reported once per layer: every report of it must agree
    for j in range(n):
        assert at[j] == at[j % len(ROLES)] or j % len(ROLES) >= 4
    return size, {key(j): at[j] for j in range(n) if at[j] >= 0}, {key(j): sc[j] for j in range(n) if sc[j] >= 0}


@pytest.mark.parametrize("n_layers", (1, 3))
@pytest.mark.parametrize("family,weight_dtype", CASES, ids=[f"{f}-{w}" for f, w in CASES])
def test_python_and_c_agree_on_every_index(family, weight_dtype, n_layers):
    lib = _lib_or_skip()
    dims = llama_dims(replace(BASE, n_layers=n_layers, **FAMILIES[family]), 2)
    fp8 = weight_dtype == "fp8"
    layout = ops.WeightTable(dims, fp8)
    size, at, sc = library_layout(lib, dims, int(fp8))
    assert size == len(layout)
    ours = {(e.name, e.layer): i for i, e in enumerate(layout) if not e.name.endswith(" scale")}
    ours_sc = {(e.name[:-len(" scale")], e.layer): i for i, e in enumerate(layout) if e.name.endswith(" scale")}
    assert at == ours and sc == ours_sc
    assert sorted(list(at.values()) + list(sc.values())) == list(range(size))  # every slot named exactly once
    for (name, layer), i in at.items():
        assert layout.index(name, layer) == i
    for (name, layer), i in sc.items():
        assert layout.scale_index(name, layer) == i


def test_the_c_query_refuses_bad_dims_and_plans():
    lib = _lib_or_skip()
    good = llama_dims(BASE, 2)
    n = len(ROLES) * 2
    at, sc = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    call = lambda d, w8, cap=n: lib.p2pt_llama_weight_layout(ctypes.byref(d), ctypes.byref(ops.WeightPlan(w8=w8)), at,
                                                               sc, cap)
    assert call(good, 0) == 3 + 6 * 2 and call(good, 1) == 3 + 6 * 2 + 9
    assert call(good, 2) == -1 and call(good, -1) == -1  # a bad WeightPlan
    assert call(good, 0, n - 1) == -1  # arrays too small
    both = llama_dims(replace(BASE, qkv_bias=True), 2)
    both.qk_norm = 1
    for bad in (both, llama_dims(replace(BASE, head_dim=32), 2), llama_dims(replace(BASE, n_kv_heads=0), 2),
                llama_dims(replace(BASE, n_layers=0), 2)):
        assert call(bad, 0) == -1


# ---------------------------------------------------------------- refusals, before any device is needed
def _build(m, table):
    return ops.FusedLlamaDecoder(m.dims(), table, m.k_cache, m.v_cache, weight_fp8=m.weight_dtype == "fp8")


def _with(table, i, t):
    return table[:i] + [t] + table[i + 1:]


BF16_ENTRIES = [("embed", None), ("final_norm", None), ("lm_head", None), ("wqkv", 1), ("wo", 1), ("w_gate_up", 1),
                ("w_down", 1)]


@pytest.mark.parametrize("name,layer", BF16_ENTRIES, ids=[n for n, _ in BF16_ENTRIES])
@pytest.mark.parametrize("family", ("plain", "rope_qk_norm"))
def test_a_wrong_shaped_bf16_weight_is_refused_by_name(family, name, layer):
    m = model(family, "bf16")
    table = m.fused_weights()
    i = ops.WeightTable(m.dims()).index(name, layer)
    where = name if layer is None else f"layer {layer}: {name}"
    bad = [table[i][:-1].contiguous()] + ([table[i].T.contiguous()] if table[i].dim() == 2 else [])
    assert all(b.shape != table[i].shape for b in bad[:1])
    for t in bad:
        if t.shape == table[i].shape:  # the transpose of a square weight keeps its shape: nothing to refuse
            continue
        with pytest.raises(ValueError, match=f"^{where} has shape"):
            _build(m, _with(table, i, t))


@pytest.mark.parametrize("weight_dtype", FORMATS)
def test_a_valid_table_passes_every_host_check(weight_dtype):
    """CPU tensors: everything judged from dtypes, shapes and the length passes, and the first refusal is the
    device's (on a host with a GPU too: the table is not on it)."""
    for family in FAMILIES:
        m = model(family, weight_dtype)
        with pytest.raises(ValueError, match="^embed must be on a HIP device"):
            _build(m, m.fused_weights())


def test_the_fp8_refusals_come_from_the_same_walk():
    m = model("rope_qkv_bias", "fp8")
    table, layout = m.fused_weights(), ops.WeightTable(m.dims(), True)
    wq, sq = layout.index("wqkv", 1), layout.scale_index("wqkv", 1)
    with pytest.raises(TypeError, match="^layer 1: wqkv: weight_fp8 is set"):
        _build(m, _with(table, wq, table[wq].to(BF)))
    with pytest.raises(TypeError, match="^lm_head: weight_fp8 is set"):
        _build(m, _with(table, 2, table[2].to(torch.float16)))
    with pytest.raises(ValueError, match="^layer 1: wqkv has shape"):
        _build(m, _with(table, wq, table[wq][:-16].contiguous()))
    with pytest.raises(ValueError, match="^layer 1: wqkv scale has shape.*one fp32 scale per output row"):
        _build(m, _with(table, sq, table[sq][:-1].contiguous()))
    with pytest.raises(TypeError, match="^layer 1: wqkv scale: expected torch.float32"):
        _build(m, _with(table, sq, table[sq].double()))
    with pytest.raises(ValueError, match="^lm_head scale has shape"):
        _build(m, _with(table, layout.scale_index("lm_head"), table[sq]))
    with pytest.raises(ValueError, match="^layer 0: bqkv has shape"):
        _build(m, _with(table, layout.index("bqkv", 0), table[layout.index("bqkv", 0)][:-2].contiguous()))
    with pytest.raises(ValueError, match="^inv_freq has shape"):
        _build(m, _with(table, 3, table[3][:-2].contiguous()))
    with pytest.raises(TypeError, match="^inv_freq: expected torch.float32"):
        _build(m, _with(table, 3, table[3].to(BF)))
    with pytest.raises(ValueError, match="weight table.*inv_freq.*7 per layer.*fp32 row scales"):
        _build(m, table[:-1])
    n = len(table) - 9
    bf = model("rope_qkv_bias", "bf16")
    with pytest.raises(TypeError, match="^lm_head is torch.float8_e4m3fn: an FP8 weight table needs weight_fp8=True"):
        _build(bf, table[:n])
    with pytest.raises(ValueError, match="weight table"):
        _build(bf, table)
    # the norm slots the kernels do not read are held to (dim,) too, and the cache's format still comes first
    with pytest.raises(ValueError, match="^layer 1: ffn_norm has shape"):
        _build(m, _with(table, layout.index("ffn_norm", 1), table[layout.index("ffn_norm", 1)][:-1].contiguous()))
    with pytest.raises(TypeError, match="needs dims.kv_fp8 = 1"):
        ops.FusedLlamaDecoder(m.dims(), [], m.k_cache.to(torch.float8_e4m3fn), m.v_cache, weight_fp8=True)


if __name__ == "__main__":  # the recording run (see the module docstring)
    print("GOLDEN = {")
    for f, w in CASES:
        print(f"    ({f!r}, {w!r}): [")
        for line in digests(model(f, w).fused_weights()):
            print(f"        {line!r},")
        print("    ],")
    print("}")
