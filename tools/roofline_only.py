"""Run only the roofline microbenchmarks of bench.py (for rocprofv3 --pmc passes).
    python tools/roofline_only.py            the layer kernel, the decode attention and the decode GEMM (tools/pmc_record.py)
    python tools/roofline_only.py cross-kv   the cross-attention K/V projection on gemm256 (tools/pmc_gemm256_record.py)"""
import json
import sys

import torch

sys.path.insert(0, ".")
import dimx  # noqa
from dimx import roofline

dev = torch.device("cuda:0")
if sys.argv[1:] == ["cross-kv"]:
    print(roofline.cross_kv_gemm(256, 300, "bf16", dev, iters=6))
    sys.exit(0)
print(json.dumps({"layer": roofline.layer_chain(256, 300, dev, iters=20),
                  "attn": roofline.decode_attention(256, 300, "bf16", dev, iters=20),
                  "gemm": roofline.decode_gemm(256, "bf16", dev, iters=20)}))
