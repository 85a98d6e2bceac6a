"""Device time of policy distillation (brl_amd/distill.py, include/brl_distill.h).

    python scripts/distill_throughput.py [out.json]      (default: profiles/distill/throughput.json)

* ``kernels``: brl_distill_targets (K = 1 and 4) and brl_distill_loss (with the gradient, and metrics only) per launch at B = 1024,
  4096 and 262 144 rows, each beside a device-to-device copy of the bytes it has to move (the yardstick);
* ``loss_head``: brl_distill_loss with the gradient against the torch composition of the same loss and its autograd
  (log_softmax, kl_div, mse_loss, backward to the logits and the value) at the same B;
* ``iteration``: the phases of one iteration at 8192 envs x 32 steps (rollout by the teacher, teacher forwards, targets, one epoch
  of B = 1024 minibatches) for a FAIR and a DeepMind student, the teacher a 4 x 1024 DeepMind network.

The methods of one group alternate inside one process: one warm-up each, then three rounds; a figure is the median (min .. max) of
the three.  Kernel figures are us per launch from HIP events around 50 back-to-back launches."""
import json
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import brl_amd  # noqa: E402
from brl_amd import distill, sl  # noqa: E402
from brl_amd.models import make_forward_pass  # noqa: E402

DEV = "cuda:0"
LAUNCHES = 50


def alternate(methods, inner=1):
    """{name: fn} -> {name: {"median", "min", "max", "runs"}} in ms per call of fn / inner: one warm-up each, then three rounds in
    which the methods take turns"""
    for fn in methods.values():
        fn()
    runs = {name: [] for name in methods}
    for _ in range(3):
        for name, fn in methods.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            runs[name].append(e0.elapsed_time(e1) / inner)
    return {name: {"median": statistics.median(r), "min": min(r), "max": max(r), "runs": r} for name, r in runs.items()}


def many(fn):
    def run():
        for _ in range(LAUNCHES):
            fn()
    return run


def us(stats):
    return {k: (v * 1e3 if not isinstance(v, list) else [x * 1e3 for x in v]) for k, v in stats.items()}


def kernel_group(B, K):
    gen = torch.Generator(device=DEV).manual_seed(B + K)
    r = lambda *s: torch.randn(s, generator=gen, device=DEV) * 3     # noqa: E731
    heads, own = r(K, B, 39), r(B, 39)
    mask = (torch.rand((B, 38), generator=gen, device=DEV) < 0.4).to(torch.uint8)
    mask[:, 0] = 1
    w = torch.from_numpy(distill.mixture_weights(None, K)).to(DEV)
    q, vstar, hq = torch.empty((B, 38), device=DEV), torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    dz, du, out = torch.empty((B, 38), device=DEV), torch.empty(B, device=DEV), torch.empty(8, device=DEV)
    work = torch.empty(distill.work_doubles(B), dtype=torch.float64, device=DEV)
    tl, tv, z, u = heads[:, :, :38], heads[:, :, 38], own[:, :38], own[:, 38]
    targets = lambda: distill.distill_targets(tl, tv, w, mask, 1.0, q, vstar, hq)     # noqa: E731
    targets()
    grad = lambda: distill.distill_loss(z, u, q, vstar, hq, mask, 1.0, 1.0, 0.5, dz, du, out, work)     # noqa: E731
    only = lambda: distill.distill_loss(z, u, q, vstar, hq, mask, 1.0, 1.0, 0.5, None, None, out, work)     # noqa: E731
    # bytes: the teachers' heads, the mask and q / vstar / hq | the student's heads, q / vstar / hq, the mask, dz / du
    nb = {"targets": B * (K * 39 * 4 + 38 + 40 * 4), "loss_grad": B * (39 * 4 + 40 * 4 + 38 + 39 * 4), "loss_metrics": B * (39 * 4 + 40 * 4 + 38)}
    copies = {}
    for name, n in nb.items():
        src = torch.empty(max(1, n // 2), dtype=torch.uint8, device=DEV)
        dst = torch.empty_like(src)
        copies["copy_" + name] = many(lambda s=src, d=dst: d.copy_(s))
    res = alternate({"targets": many(targets), "copy_targets": copies["copy_targets"], "loss_grad": many(grad),
                     "copy_loss_grad": copies["copy_loss_grad"], "loss_metrics": many(only), "copy_loss_metrics": copies["copy_loss_metrics"]},
                    inner=LAUNCHES)
    out_ = {"B": B, "K": K}
    for name, n in nb.items():
        k, c = us(res[name]), us(res["copy_" + name])
        out_[name] = {"us_per_launch": k, "bytes": n, "GB_per_s": n / k["median"] / 1e3, "copy_us": c, "launch_over_copy": k["median"] / c["median"]}
    return out_


def loss_head(B):
    F = torch.nn.functional
    gen = torch.Generator(device=DEV).manual_seed(B)
    heads, own = torch.randn((1, B, 39), generator=gen, device=DEV) * 3, torch.randn((B, 39), generator=gen, device=DEV) * 3
    mask = torch.rand((B, 38), generator=gen, device=DEV) < 0.4
    mask[:, 0] = True
    w = torch.ones(1, device=DEV)
    q, vstar, hq = torch.empty((B, 38), device=DEV), torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    dz, du, out = torch.empty((B, 38), device=DEV), torch.empty(B, device=DEV), torch.empty(8, device=DEV)
    work = torch.empty(distill.work_doubles(B), dtype=torch.float64, device=DEV)
    distill.distill_targets(heads[:, :, :38], heads[:, :, 38], w, mask, 1.0, q, vstar, hq)
    neg = torch.finfo(torch.float32).min

    def composition():
        z, u = own[:, :38].clone().requires_grad_(True), own[:, 38].clone().requires_grad_(True)
        logp = torch.log_softmax(torch.where(mask, z, torch.full_like(z, neg)), dim=-1)
        loss = F.kl_div(logp, q, reduction="none").sum(-1).mean() + 0.5 * F.mse_loss(u, vstar)
        loss.backward()

    kernel = lambda: distill.distill_loss(own[:, :38], own[:, 38], q, vstar, hq, mask, 1.0, 1.0, 0.5, dz, du, out, work)     # noqa: E731
    res = alternate({"kernel": many(kernel), "torch_composition": many(composition)}, inner=LAUNCHES)
    return {"B": B, "kernel_us": us(res["kernel"]), "torch_composition_us": us(res["torch_composition"]),
            "composition_over_kernel": res["torch_composition"]["median"] / res["kernel"]["median"]}


def iteration(model, env, teacher, N=8192, T=32, B=1024):
    fp_t = make_forward_pass("relu", "DeepMind")
    roll = brl_amd.make_roll_out(dict(num_steps=T, reward_scale=7600.0, game_mode="competitive", actor_illegal_action_mask=True), env, fp_t, fp_t)
    n = N * T
    student = make_forward_pass("relu", model).init(2, device=DEV)
    step = distill.DistillStep(student, sl.make_optimizer(student, 1e-4), B, n)
    heads = torch.empty((1, n, 39), dtype=torch.float32, device=DEV)
    w = torch.ones(1, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(3)
    st = env.init(4, num_envs=N)
    box = {}

    def rollout():
        _, box["traj"] = roll((teacher, None, st, st.observation, 0, 0), teacher)

    def load():
        step.data_obs.copy_(box["traj"].obs.reshape(n, 480))
        step.data_mask.copy_(box["traj"].legal_action_mask.reshape(n, 38))

    rollout()
    load()
    res = alternate({"rollout": rollout, "load": load, "teacher_forwards": lambda: distill.teacher_heads([teacher], step.data_obs, heads),
                     "targets": lambda: distill.distill_targets(heads[:, :, :38], heads[:, :, 38], w, step.data_mask, 1.0, step.data_q,
                                                                step.data_vstar, step.data_hq),
                     "epoch": lambda: step.epoch(n, gen)})
    return {"student": model, "num_envs": N, "num_steps": T, "minibatch_size": B, "steps_per_epoch": n // B, "ms": res}


if __name__ == "__main__":
    out = {"device": torch.cuda.get_device_name(0), "block": distill.BLOCK, "kernels": [], "loss_head": [], "iteration": []}
    for B in (1024, 4096, 262144):
        for K in (1, 4):
            out["kernels"].append(kernel_group(B, K))
    for B in (1024, 4096):
        out["loss_head"].append(loss_head(B))
    d = np.load(os.path.join(HERE, "tests", "golden", "wb5_dds_1000.npz"))
    env = brl_amd.BridgeBidding(lut=(d["keys"], d["values"]), device=DEV)
    teacher = make_forward_pass("relu", "DeepMind").init(1, device=DEV)
    for model in ("FAIR", "DeepMind"):
        out["iteration"].append(iteration(model, env, teacher))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "distill", "throughput.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out, indent=1))
