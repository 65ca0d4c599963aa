"""Request-level prosody controls (speed, pitch, energy, exaggeration) and their mapping onto
the engine's per-utterance controls (include/tts_hip.h, tts_prosody).  Host arithmetic only: the
model and the service both validate a request here, before anything is queued or launched."""
from __future__ import annotations

from typing import Optional

import numpy as np

# public ranges of the request-level controls
SPEED_RANGE = (0.25, 4.0)
SHIFT_RANGE = (-4.0, 4.0)
EXAGGERATION_NEUTRAL = 0.5


def prosody_controls(speed=1.0, pitch=0.0, energy=0.0, exaggeration=EXAGGERATION_NEUTRAL) -> Optional[dict]:
    """The request-level controls -> the engine's (a dict of engine.PROSODY_FIELDS scalars), or None
    when all are neutral:
        duration_scale = float32(1) / float32(speed), speed in [0.25, 4] (the speaking rate)
        pitch_shift = pitch, energy_shift = energy, each in [-4, 4]
        pitch_range = energy_range = clip(2 * exaggeration, 0, 4); exaggeration 0.5 is neutral
    A value that is no number, not finite or (speed, pitch, energy) outside its range raises
    ValueError naming the field."""
    vals = {}
    for name, v in (("speed", speed), ("pitch", pitch), ("energy", energy), ("exaggeration", exaggeration)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a number, got {type(v).__name__}")
        v = float(v)
        if not np.isfinite(v):
            raise ValueError(f"{name} must be finite, got {v}")
        vals[name] = v
    if not SPEED_RANGE[0] <= vals["speed"] <= SPEED_RANGE[1]:
        raise ValueError(f"speed {vals['speed']} outside [{SPEED_RANGE[0]}, {SPEED_RANGE[1]}]")
    for name in ("pitch", "energy"):
        if not SHIFT_RANGE[0] <= vals[name] <= SHIFT_RANGE[1]:
            raise ValueError(f"{name} {vals[name]} outside [{SHIFT_RANGE[0]}, {SHIFT_RANGE[1]}]")
    rng = float(np.clip(2.0 * vals["exaggeration"], 0.0, 4.0))
    out = {"duration_scale": float(np.float32(1) / np.float32(vals["speed"])), "pitch_shift": vals["pitch"],
           "pitch_range": rng, "energy_shift": vals["energy"], "energy_range": rng}
    if vals["speed"] == 1.0 and vals["pitch"] == 0.0 and vals["energy"] == 0.0 and rng == 1.0:
        return None
    return out
