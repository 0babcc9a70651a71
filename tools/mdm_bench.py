#!/usr/bin/env python3
"""ms per ``gen_sequence`` of the motion generator (default-size model, weights from a seed, guidance on, 3 DDIM steps: stride 10 of 21
timesteps) at batch sizes 32, 1 024 and 4 096, with the per-kernel split (hipEvents), against the CPU restatement ``tests/mdm_ref.py``
moved to the same GPU under torch (eval arithmetic, ``no_grad``): the baseline is never the code under test.
Each side is timed ``repeats`` times after a warm-up, with a device synchronisation around every timed call; a side wins when every one of
its runs lies below every run of the other and the gap of the medians is at least three times the larger spread (section 9's rule).
Prints one JSON line per batch size.

    python tools/mdm_bench.py [repeats] [batch sizes, comma-separated]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mdm_ref as R  # noqa: E402
from parc_amd import motion_generator as mg  # noqa: E402

DEV = "cuda:0"
STRIDE, SCALE = 10, 1.5


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    sizes = [int(s) for s in sys.argv[2].split(",")] if len(sys.argv) > 2 else [32, 1024, 4096]
    cfg = mg.default_config()
    sd = mg.random_state_dict(cfg, 0)
    g = torch.Generator().manual_seed(1)
    mean, std = torch.randn((15, 91), generator=g) * 0.3, torch.rand((15, 91), generator=g) * 1.5 + 0.5
    ref = R.MdmRef(cfg, sd, mean, std, torch.float32, DEV)
    for n in sizes:
        gen = mg.MDMGenerator.from_state_dict(cfg, sd, mean, std, DEV, max_batch=n)
        c = R.random_conds(n, 2, 91, 2, flags=[(1, 1, 1, 1)] * n)
        c = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
        x = torch.randn((n, 15, 91), generator=g).to(DEV)
        prev = gen.extract_motion_features(c["prev"])
        hf_m = c["hf"] * gen.max_h

        def hip():
            k = dict(R.to_keys(R.copy_conds(c)), OBS_KEY=hf_m, PREV_STATE_KEY=prev, GUIDANCE_PARAMS=mg.GuidanceParams(SCALE))
            return gen.gen_sequence(k, STRIDE, "DDIM", noise=x)

        def base():
            with torch.no_grad():
                rc = dict(R.copy_conds(c), scale=SCALE, hf=torch.clamp(hf_m, -gen.max_h, gen.max_h) / gen.max_h, prev=gen.assemble_mdm_features(prev))
                return gen.extract_motion_features(ref.gen_sequence_features(rc, x, STRIDE, "DDIM"))

        a, b = hip(), base()
        diff = max((a[k] - b[k]).abs().max().item() for k in a)
        timed(hip, 2), timed(base, 2)
        th, kts = [], []
        for _ in range(reps):
            th += timed(hip, 1)
            kts.append(gen.kernel_times())
        tb = timed(base, reps)
        kt = {k: round(float(np.median([q[k] for q in kts])), 4) for k in mg.KERNELS}
        mh, mb = float(np.median(th)), float(np.median(tb))
        spread = max(max(th) - min(th), max(tb) - min(tb))
        fast, slow = (th, tb) if mh < mb else (tb, th)
        print(json.dumps({"batch": n, "steps": 3, "guidance": True, "hip_ms": round(mh, 3), "hip_min_max": [round(min(th), 3), round(max(th), 3)],
                          "torch_ms": round(mb, 3), "torch_min_max": [round(min(tb), 3), round(max(tb), 3)], "kernel_ms": kt,
                          "ms_kernels": round(sum(kt.values()), 3), "speedup": round(mb / mh, 2),
                          "separated": bool(max(fast) < min(slow) and abs(mb - mh) >= 3 * spread), "max_abs_diff": diff,
                          **{k: v for k, v in gen.describe().items()}}), flush=True)
        del gen


if __name__ == "__main__":
    main()
