"""Writes tests/golden/extreme_draws.json: (seed, env_id, draw) triples whose 24-bit action draw
(orc_action_draw(seed, env_id, draw) >> 8) is one of the four ends of the range: 2**24 - 1, 2**24 - 2, 1, 0.

    python tests/golden/make_extreme_draws.py

A vectorised numpy restatement of Philox4x32-10 as oracle/bridge_oracle.c keys it for the action stream scans
2**15 envs x 2**12 draws (about eight hits per value); tests/test_categorical_host.py checks every committed triple
through the oracle itself."""
import json
import os

import numpy as np

SEED = 19
ENV0, NENV = 1000, 1 << 15      # env ids >= 1000: room for the env_offset = env_id - j of the GPU test
NDRAW = 1 << 12
STREAM_ACTION = 0x42524C41
WANT = {"top": (1 << 24) - 1, "top_minus_1": (1 << 24) - 2, "one": 1, "zero": 0}
KEEP = 4                        # triples kept per value
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def action_draws(seed, env_ids, block):
    """the four draws 4 * block .. 4 * block + 3 of every env: [4, len(env_ids)] uint32"""
    env_ids = np.asarray(env_ids, dtype=np.uint64)
    out = philox4x32_10(env_ids & M32, np.full_like(env_ids, block), np.full_like(env_ids, STREAM_ACTION),
                        env_ids >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(out).astype(np.uint32)


def main():
    envs = np.arange(ENV0, ENV0 + NENV, dtype=np.uint64)
    found = {name: [] for name in WANT}
    for block in range(NDRAW // 4):
        u24 = action_draws(SEED, envs, block) >> 8
        for name, v in WANT.items():
            for sel, e in zip(*np.nonzero(u24 == v)):
                found[name].append({"seed": SEED, "env_id": int(envs[e]), "draw": 4 * block + int(sel), "u24": v})
    out = {name: sorted(rows, key=lambda r: (r["draw"], r["env_id"]))[:KEEP] for name, rows in found.items()}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "extreme_draws.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print({k: len(v) for k, v in found.items()}, "->", path)


if __name__ == "__main__":
    main()
