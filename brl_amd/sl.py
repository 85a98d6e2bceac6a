"""Supervised pre-training from recorded auctions: the reference's ``sl.py`` on the GPU.

``python -m brl_amd.sl data_path=DIR save_path=DIR [key=value ...]`` (the names and defaults of ``SLConfig``, sl.py:52-81).
Every ``eval_every`` steps it writes ``save_path/params-{1+step}.pkl``, a pickled Haiku tree that ``brl_amd.train`` takes as
``initial_model_path`` / ``eval_opp_model_path`` (``checkpoint.load_params(..., ".pkl")``).

The batch is made on the device (include/brl_sl.h): ``brl_sl_sample`` draws the (trajectory, call index) pairs of the example
stream, ``brl_sl_replay`` deals and re-bids them into observation rows, legal masks and labels, ``brl_sl_loss`` forms the loss,
the metrics and d loss / d logits; torch differentiates the network's layers only.  ``SLStep`` captures S such steps (sample,
replay, forward, loss, backward, Adam, the post-update accuracy) in one hipGraph; the host touches nothing between them and
reads the per-step metrics only when it logs.
"""
from __future__ import annotations

import os
import pickle
import sys
import time

import numpy as np
import torch

from . import _capi, checkpoint
from ._capi import device_index, stream
from ._capture import capture_each, preserved, warm_up
from .models import make_forward_pass
from .sl_data import CALL_NAMES, TrajectorySet, decision_points, hand_string, load_trajectories

SL_DEFAULTS = dict(  # sl.py:52-81 (SLConfig), same names and defaults
    iterations=400000, train_batch=128, learning_rate=1e-4, eval_every=10000, data_path=None, save_path=None, num_examples=3,
    eval_batch=10000, rng_seed=42, entropy_coef=0.0, type_of_model="DeepMind", activation="relu",
)

MISSING_DATA_HINT = ("Please generate your own supervised training data or download from "
                     "https://console.cloud.google.com/storage/browser/openspiel-data/bridge"
                     " and supply the local location as --data_path")   # sl.py:256-262

TOP_K_ACTIONS = 5


class DeviceSet:
    """a TrajectorySet on the GPU (hands as int64: the same 64 bits)"""

    def __init__(self, ts: TrajectorySet, device):
        self.host = ts
        self.n = ts.n
        self.hands = torch.from_numpy(ts.hands.view(np.int64).copy()).to(device)
        self.offsets = torch.from_numpy(ts.offsets.astype(np.int64)).to(device)
        self.calls = torch.from_numpy(ts.calls.astype(np.uint8)).to(device)


# ---- the three entry points ---------------------------------------------------------------------------------------------------
def sl_sample(data: DeviceSet, counter: torch.Tensor, seed: int, traj: torch.Tensor, pos: torch.Tensor) -> None:
    di = device_index(traj)
    _capi.check(_capi.lib().brl_sl_sample(di, counter.data_ptr(), data.offsets.data_ptr(), data.n, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           traj.shape[0], traj.data_ptr(), pos.data_ptr(), stream(di)))


def sl_replay(data: DeviceSet, traj, pos, obs, mask, label) -> None:
    di = device_index(obs)
    _capi.check(_capi.lib().brl_sl_replay(di, data.hands.data_ptr(), data.offsets.data_ptr(), data.calls.data_ptr(), data.n,
                                           _capi.ptr(traj), _capi.ptr(pos), traj.shape[0], _capi.ptr(obs), _capi.ptr(mask),
                                           _capi.ptr(label), stream(di)))


def sl_loss(logits, label, mask, ent_coef: float, dlogits, out, counter=None, advance: int = 0) -> None:
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    di = device_index(logits)
    _capi.check(_capi.lib().brl_sl_loss(di, logits.data_ptr(), logits.stride(0), _capi.ptr(label), _capi.ptr(mask), label.shape[0],
                                         float(ent_coef), _capi.ptr(dlogits), out.data_ptr(),
                                         None if counter is None else counter.data_ptr(), int(advance), stream(di)))


def make_optimizer(net: torch.nn.Module, learning_rate: float):
    """optax.adam(learning_rate) (sl.py:160): b1 0.9, b2 0.999, eps 1e-8, no clipping, no schedule"""
    return torch.optim.Adam(net.parameters(), lr=learning_rate, betas=(0.9, 0.999), eps=1e-8, fused=True, capturable=True)


class Batch:
    """static device buffers of one batch of examples"""

    def __init__(self, b: int, device):
        self.traj = torch.zeros(b, dtype=torch.int64, device=device)
        self.pos = torch.zeros(b, dtype=torch.int32, device=device)
        self.obs = torch.zeros((b, 480), dtype=torch.float32, device=device)
        self.mask = torch.zeros((b, 38), dtype=torch.uint8, device=device)
        self.label = torch.zeros(b, dtype=torch.int32, device=device)


class SLStep:
    """S training steps per hipGraph replay (sl.py:186-197, 268-279).  One step: sample + replay a batch of the train stream,
    forward, brl_sl_loss with the gradient (metrics row ``pre[s]``: total, target_loss, entropy — before the update), backward
    through the layers, Adam, a no-grad forward and brl_sl_loss metrics-only (``post[s]``: the accuracy after the update,
    sl.py:275-279), which also advances the stream's counter.  A run of k < S steps replays a 1-step graph k times."""

    def __init__(self, net, opt, data: DeviceSet, batch: int, seed: int, entropy_coef: float, steps_per_graph: int = 8, graph=True):
        self.net, self.opt, self.data = net, opt, data
        self.B, self.seed, self.ent, self.S = int(batch), int(seed), float(entropy_coef), int(steps_per_graph)
        dev = next(net.parameters()).device
        self.b = Batch(self.B, dev)
        self.dlogits = torch.zeros((self.B, 38), dtype=torch.float32, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.pre = torch.zeros((self.S, 5), dtype=torch.float32, device=dev)
        self.post = torch.zeros((self.S, 5), dtype=torch.float32, device=dev)
        self.graphs = {}
        if graph:
            self._capture()

    def _step(self, s: int):
        b = self.b
        sl_sample(self.data, self.counter, self.seed, b.traj, b.pos)
        sl_replay(self.data, b.traj, b.pos, b.obs, b.mask, b.label)
        logits, _ = self.net(b.obs)
        sl_loss(logits, b.label, b.mask, self.ent, self.dlogits, self.pre[s])
        self.opt.zero_grad(set_to_none=False)
        torch.autograd.backward(logits, self.dlogits)
        self.opt.step()
        with torch.no_grad():
            logits2, _ = self.net(b.obs)
        sl_loss(logits2, b.label, b.mask, self.ent, None, self.post[s], self.counter, self.B)

    def _steps(self, k: int):
        for s in range(k):
            self._step(s)

    def _capture(self):
        # warm-up and capture run the real step: parameters, optimizer state and the stream counter are put back afterwards
        ks = sorted({1, self.S})
        with preserved(self.net.parameters(), self.opt, tensors=(self.counter,)):
            warm_up(lambda: self._step(0), 3)
            self.graphs = dict(zip(ks, capture_each([lambda k=k: self._steps(k) for k in ks])))

    def run(self, k: int):
        """k <= S steps: one S-step replay when k == S, else k 1-step replays.  Returns the device metrics rows [k, 4] (total,
        target_loss, entropy before each update; accuracy after it); reading them is the caller's choice."""
        assert 1 <= k <= self.S
        if k == self.S:
            self.graphs[self.S].replay()
            return torch.cat([self.pre[:, :3], self.post[:, 3:4]], dim=1)
        rows = []
        for _ in range(k):
            self.graphs[1].replay()
            rows.append(torch.cat([self.pre[:1, :3], self.post[:1, 3:4]], dim=1))
        return torch.cat(rows)

    def eager(self, k: int):
        """the same k steps without graphs (the composition the graphs are checked against)"""
        rows = []
        for _ in range(k):
            self._step(0)
            rows.append(torch.cat([self.pre[:1, :3], self.post[:1, 3:4]], dim=1))
        return torch.cat(rows)


# ---- evaluation ---------------------------------------------------------------------------------------------------------------
def evaluate_pairs(net, data: DeviceSet, traj: torch.Tensor, pos: torch.Tensor, entropy_coef: float = 0.0, chunk: int = 65536):
    """metrics of explicit examples (the pairs' mean): dict with total_loss, target_loss, entropy, accuracy, illegal_actions_prob"""
    dev = traj.device
    n = traj.shape[0]
    acc = np.zeros(5)
    out = torch.zeros(5, dtype=torch.float32, device=dev)
    for i in range(0, n, chunk):
        t, p = traj[i:i + chunk].contiguous(), pos[i:i + chunk].contiguous()
        b = Batch(t.shape[0], dev)
        sl_replay(data, t, p, b.obs, b.mask, b.label)
        with torch.no_grad():
            logits, _ = net(b.obs)
        sl_loss(logits, b.label, b.mask, entropy_coef, None, out)
        acc += out.double().cpu().numpy() * t.shape[0]
    m = acc / n
    return dict(zip(("total_loss", "target_loss", "entropy", "accuracy", "illegal_actions_prob"), m.tolist()))


def evaluate_all(net, data: DeviceSet, entropy_coef: float = 0.0):
    """the metrics over every decision point of a set"""
    traj, pos = decision_points(data.host)
    dev = data.hands.device
    return evaluate_pairs(net, data, torch.from_numpy(traj).to(dev), torch.from_numpy(pos).to(dev), entropy_coef)


class EvalStream:
    """the test stream (sl.py:288-300): the next eval_batch examples, its own seed and counter"""

    def __init__(self, data: DeviceSet, batch: int, seed: int):
        self.data, self.seed = data, int(seed)
        dev = data.hands.device
        self.b = Batch(int(batch), dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.out = torch.zeros(5, dtype=torch.float32, device=dev)

    def next(self, net, entropy_coef: float):
        b = self.b
        sl_sample(self.data, self.counter, self.seed, b.traj, b.pos)
        sl_replay(self.data, b.traj, b.pos, b.obs, b.mask, b.label)
        with torch.no_grad():
            logits, _ = net(b.obs)
        sl_loss(logits, b.label, b.mask, entropy_coef, None, self.out, self.counter, b.traj.shape[0])
        m = self.out.cpu().numpy().tolist()
        return {"test/total_loss": m[0], "test/target_loss": m[1], "test/entropy": m[2], "test/test_accuracy": m[3],
                "test/illegal_actions_prob": m[4]}


def output_samples(net, data: DeviceSet, max_samples: int, rng: np.random.RandomState, out=print):
    """sl.py:207-240: test positions where the net's choice differs from the data — the hand of the seat to act, the auction so
    far, the top 5 calls of the unmasked policy and the ground truth (plain text, not pyspiel's rendering)."""
    if max_samples <= 0:
        return 0
    ts, dev = data.host, data.hands.device
    count = 0
    for t in rng.permutation(ts.n):
        nc = int(ts.offsets[t + 1] - ts.offsets[t])
        b = Batch(nc, dev)
        sl_replay(data, torch.full((nc,), int(t), dtype=torch.int64, device=dev), torch.arange(nc, dtype=torch.int32, device=dev),
                  b.obs, b.mask, b.label)
        with torch.no_grad():
            logits, _ = net(b.obs)
        pi = torch.softmax(logits, dim=-1).cpu().numpy()
        calls = ts.calls[ts.offsets[t]:ts.offsets[t + 1]]
        for k in range(nc):
            if int(np.argmax(pi[k])) != int(calls[k]):
                seat = k % 4
                auction = " ".join(CALL_NAMES[c] for c in calls[:k]) or "(none)"
                lines = [f"Seat {'NESW'[seat]} to call, dealer N, none vulnerable", f"  hand: {hand_string(ts.hands[t, seat])}",
                         f"  auction: {auction}"]
                for a in np.argsort(-pi[k], kind="stable")[:TOP_K_ACTIONS]:
                    lines.append(f"{CALL_NAMES[a]:7} {pi[k][a]:.2f}")
                lines.append(f"Ground truth {CALL_NAMES[calls[k]]}\n")
                out("\n".join(lines))
                count += 1
                break
        if count >= max_samples:
            break
    return count


def save_pickle(net, path: str) -> None:
    """``pickle.dump(params)`` of the reference (sl.py:303-306): the Haiku tree of the network, numpy leaves"""
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        pickle.dump(checkpoint.torch_to_haiku(net), f)
    os.replace(tmp, path)


# ---- the loop -----------------------------------------------------------------------------------------------------------------
def load_data(config, log=print):
    """train and test sets, or the reference's hint on stderr and exit 1 (sl.py:245-264)"""
    try:
        if config["data_path"] is None:
            raise FileNotFoundError("data_path is not set")
        train = load_trajectories(os.path.join(config["data_path"], "train.txt"), log)
        test = load_trajectories(os.path.join(config["data_path"], "test.txt"), log)
    except OSError as e:
        print(e, file=sys.stderr)
        print(MISSING_DATA_HINT, file=sys.stderr)
        sys.exit(1)
    return train, test


def train_sl(config, log=print, steps_per_graph: int = 8, device=None):
    """sl.py:main: returns the trained module.  ``log`` receives the metric dicts (sl.py:281-311), one per step and one per
    evaluation."""
    cfg = dict(SL_DEFAULTS)
    cfg.update(config)
    train_ts, test_ts = load_data(cfg, log)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    net = make_forward_pass(cfg["activation"], cfg["type_of_model"]).init(int(cfg["rng_seed"]), device=dev)
    opt = make_optimizer(net, float(cfg["learning_rate"]))
    train, test = DeviceSet(train_ts, dev), DeviceSet(test_ts, dev)
    seed = int(cfg["rng_seed"])
    step = SLStep(net, opt, train, int(cfg["train_batch"]), seed, float(cfg["entropy_coef"]), steps_per_graph)
    evals = EvalStream(test, int(cfg["eval_batch"]), seed + 1)
    rng = np.random.RandomState(seed)
    iters, every = int(cfg["iterations"]), int(cfg["eval_every"])
    i = 0
    t0 = time.perf_counter()
    while i < iters:
        k = min(step.S, iters - i, every - i % every)
        rows = step.run(k).cpu().numpy()
        for r in range(k):
            metrics = {"step": i + r, "train/total_loss": float(rows[r, 0]), "train/target_loss": float(rows[r, 1]),
                       "train/entropy": float(rows[r, 2]), "train/train_accuracy": float(rows[r, 3])}
            if r == k - 1 and (i + k) % every == 0:
                test_metrics = evals.next(net, float(cfg["entropy_coef"]))
                print(f"After {i + k} steps, test accuracy: {test_metrics['test/test_accuracy']}.")
                if cfg["save_path"] is not None:
                    os.makedirs(cfg["save_path"], exist_ok=True)
                    save_pickle(net, os.path.join(cfg["save_path"], f"params-{i + k}.pkl"))
                output_samples(net, test, int(cfg["num_examples"]), rng)
                log({"step": i + r, **test_metrics})
            log(metrics)
        i += k
    torch.cuda.synchronize(dev)
    log({"steps": iters, "seconds": time.perf_counter() - t0})
    return net


def main(argv=None):
    from .train import parse_cli
    cfg = parse_cli(sys.argv[1:] if argv is None else argv, defaults=SL_DEFAULTS)
    print(cfg)
    train_sl(cfg)


if __name__ == "__main__":
    main()
