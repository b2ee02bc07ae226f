#!/usr/bin/env python
"""How far bf16 autocast moves the REFERENCE's own RelationalTransformerEncoderLayer stack on the `great` fixture
(tests/golden/great_great.npz: D = 64, 4 heads, L = 23, two layers): the yardstick for the bf16x1 mode of the HIP layer
(hip_ops.set_seq_gemm_mode("bf16x1"), tests/test_seq_amp_gpu.py).  CPU only; run in the build container:
    python tests/golden/make_golden_seq_amp.py
Loads the fixture's inputs and state_dict into the reference layers, runs them in fp32 and under
torch.autocast("cpu", torch.bfloat16), and writes tests/golden/seq_amp_autocast_error.json:
    output    ||y_autocast - y_fp32||_2 / ||y_fp32||_2 over the unmasked positions
    gradient  the largest ||g_autocast - g_fp32||_2 / ||g_fp32||_2 over g_x and every parameter gradient that is not all zero
(the same two figures tests/test_seq_amp_gpu.py computes for the HIP layer against the fixture's fp32 vectors)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
from buglab.models.layers.relational_transformer import RelationalTransformerEncoderLayer  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def run(z, autocast):
    D, H, layers, FF, T, value_bias, scalar = (int(v) for v in z["cfg"])
    stack = torch.nn.ModuleList([
        RelationalTransformerEncoderLayer(d_model=D, key_query_dimension=D // H, value_dimension=D // H, nhead=H, num_edge_types=T,
                                          dim_feedforward=FF, dropout=0.0, use_edge_value_biases=bool(value_bias),
                                          edge_attention_bias_is_scalar=bool(scalar), normalisation_mode=str(z["norm"]))
        for _ in range(layers)])
    stack.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p.")})
    x = torch.from_numpy(z["x"]).requires_grad_(True)
    masked = torch.from_numpy(z["masked"])
    edges, types = torch.from_numpy(z["edges"]), torch.from_numpy(z["edge_types"])
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        y = x
        for l in stack:
            y = l(y, masked, edges, types)
    y = y.float()
    (y * torch.from_numpy(z["w"]) * (~masked)[:, :, None]).sum().backward()
    grads = {"g_x": x.grad}
    grads.update({"g." + k: v.grad for k, v in stack.named_parameters() if v.grad is not None})
    return y.detach()[~masked], grads


if __name__ == "__main__":
    z = np.load(os.path.join(HERE, "great_great.npz"))
    y32, g32 = run(z, False)
    assert float((y32 - torch.from_numpy(z["y"])[~torch.from_numpy(z["masked"])]).abs().max()) < 1e-5  # the fixture's own vectors
    y16, g16 = run(z, True)
    per = {k: rel(g16[k], g32[k]) for k in g32 if float(g32[k].norm()) > 0}
    worst = max(per, key=per.get)
    out = {"fixture": "great_great.npz", "autocast": "torch.autocast('cpu', torch.bfloat16)", "torch": torch.__version__,
           "output": rel(y16, y32), "gradient": per[worst], "gradient_worst_tensor": worst}
    with open(os.path.join(HERE, "seq_amp_autocast_error.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)
    print({k: round(v, 5) for k, v in per.items()})
