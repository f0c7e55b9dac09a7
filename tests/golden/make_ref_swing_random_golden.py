"""Generates tests/golden/ref_swing_random.npz from the REFERENCE'S OWN compiled swing planner (oracle/_ref/libref_swing.so, built by
`make -C oracle ref` where the reference tree exists):

    python tests/golden/make_ref_swing_random_golden.py

What tests/test_ref_swing.py compares the host mirror with, so that the comparison needs no library: the stance legs of every mode
number, and for the 60 random schedules of random_cases() (seed 1234) whether the reference accepts the schedule and, on the 64 query
times, its active mode and per leg z, zdot, zddot and impact-proximity factor (zeros where the schedule is rejected)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED, TRIALS, TIMES = 1234, 60, 64


def random_cases(model, rng):
    """Random mode sequences (all four modes, random durations) with random planner settings: (cfg, event_times, mode_sequence, t, terrain)."""
    for trial in range(TRIALS):
        n_ev = int(rng.integers(2, 14))
        ev = np.cumsum(rng.uniform(0.05, 0.7, n_ev))
        seq = rng.integers(0, 4, n_ev + 1)
        if trial % 3:
            seq[0] = seq[-1] = 3      # most schedules start and end in stance like the reference's own
        cfg = dict(model.swing)
        cfg.update(liftOffVelocity=rng.uniform(0, 0.3), touchDownVelocity=-rng.uniform(0, 0.3), swingHeight=rng.uniform(0.02, 0.2),
                   touchDownHeightOffset=rng.uniform(-0.01, 0.01), swingTimeScale=rng.uniform(0.1, 0.6))
        terrain = rng.uniform(-0.05, 0.05)
        t = np.sort(rng.uniform(ev[0] - 0.2, ev[-1] + 0.2, TIMES))
        yield cfg, ev, seq, t, terrain


def main():
    from ref_swing import RefSwing
    from wb_humanoid_mpc_amd import load_model
    from wb_humanoid_mpc_amd.reference import MODE_BY_NAME
    model = load_model()
    ref = RefSwing()
    modes = np.array(sorted(MODE_BY_NAME.values()), dtype=np.int32)
    out = dict(mode_numbers=modes, stance_legs=np.array([ref.stance_legs(m) for m in modes]),
               ok=np.zeros(TRIALS, dtype=bool), t=np.zeros((TRIALS, TIMES)), terrain=np.zeros(TRIALS),
               values=np.zeros((TRIALS, TIMES, 2, 4)), modes=np.zeros((TRIALS, TIMES), dtype=np.int32))
    for i, (cfg, ev, seq, t, terrain) in enumerate(random_cases(model, np.random.default_rng(SEED))):
        ok, vals, md = ref.swing_planner(cfg, ev, seq, t, terrain)
        out["ok"][i], out["t"][i], out["terrain"][i] = ok, t, terrain
        if ok:
            out["values"][i], out["modes"][i] = vals, md
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_swing_random.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {int(out['ok'].sum())} accepted, {TRIALS - int(out['ok'].sum())} rejected schedules")


if __name__ == "__main__":
    main()
