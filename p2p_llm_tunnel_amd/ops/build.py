"""Compile the HIP kernels in-tree for gfx950 (CDNA4 / MI355X).

    hipcc -O3 --offload-arch=gfx950 -shared -fPIC decode_moe.o decode_w4g.o kernels.hip decode_fused.hip sample.hip \
          logprobs.hip kv_copy.hip embed_pool.hip penalty.hip guide.hip decode_lora.hip lora_delta.hip decode_f8g.hip \
          lm_score.hip -o _hip_ops.so

decode_moe.hip (the routed-expert FFN's kernels) is compiled to an object first, with the same flags and without packed
fp32 instructions (``NO_PK_F32``), and so is decode_w4g.hip (the grouped int4 instantiations of the fused GEMM, whose
decode is scalar fp32 arithmetic); every other source is compiled as it always was, so their code does not change.
decode_lora.hip (the LoRA-delta instantiations of the fused GEMM) and lora_delta.hip (k_lora_delta) are translation
units of their own with the common flags (docs/LORA.md), and so is decode_f8g.hip (the block-scaled FP8 instantiations
of the fused GEMM; docs/WEIGHT_FP8G128.md), and lm_score.hip (the prompt scorer's LM head; docs/PROMPT_LOGPROBS.md).

Cross-compiles on a CPU-only host; the .so travels with the repo snapshot to
the GPU box.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, f) for f in ("kernels.hip", "decode_fused.hip", "sample.hip", "logprobs.hip",
                                          "kv_copy.hip", "embed_pool.hip", "penalty.hip", "guide.hip",
                                          "decode_lora.hip", "lora_delta.hip", "decode_f8g.hip", "lm_score.hip")]
MOE_SRC = os.path.join(HERE, "decode_moe.hip")
W4G_SRC = os.path.join(HERE, "decode_w4g.hip")
DEPS = SRCS + [MOE_SRC, W4G_SRC] + [os.path.join(HERE, h) for h in (
    "bf16_common.h", "row_common.h", "decode_fused_kernels.h", "decode_fused_set.h", "decode_moe.h",
    "decode_moe_kernels.h", "decode_w4g.h", "decode_lora.h", "decode_f8g.h")]
NO_PK_F32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
OUT = os.path.join(HERE, "_hip_ops.so")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950").split(";")[0]


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise FileNotFoundError("hipcc not found (expected /opt/rocm/bin/hipcc)")


def up_to_date() -> bool:
    return os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in DEPS)


def build(verbose: bool = False, force: bool = False) -> str:
    if up_to_date() and not force:
        return OUT
    flags = ["-O3", f"--offload-arch={ARCH}", "-std=c++17", "-fPIC"]
    with tempfile.TemporaryDirectory(prefix="p2pt_hip_ops_") as tmp:
        moe_obj, w4g_obj = os.path.join(tmp, "decode_moe.o"), os.path.join(tmp, "decode_w4g.o")
        # The objects go ahead of the sources: hipcc's "-x hip" holds for every input after a .hip file.
        for cmd in ([hipcc(), *flags, *NO_PK_F32, "-c", MOE_SRC, "-o", moe_obj],
                    [hipcc(), *flags, *NO_PK_F32, "-c", W4G_SRC, "-o", w4g_obj],
                    [hipcc(), *flags, "-shared", "-o", OUT + ".tmp", moe_obj, w4g_obj, *SRCS]):
            if verbose:
                print(" ".join(cmd), flush=True)
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:
                raise RuntimeError("hipcc failed:\n" + r.stdout[-8000:])
    os.replace(OUT + ".tmp", OUT)
    return OUT


if __name__ == "__main__":
    print(build(verbose=True, force=True))
