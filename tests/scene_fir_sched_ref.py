"""The reference of a schedule of the scene filter mix: the existing models (tests/scene_fir_model.py, tests/scene_fir_delay_model.py,
imported unchanged) fed a step's rows CUT AT EVERY t_set, with a plain set before each piece -- the statement of the header.  The
models take pieces of any length; nothing here knows how the engine mixes a schedule."""
import numpy as np

from tests.scene_fir_delay_model import Model as DelayModel
from tests.scene_fir_model import Model as FirModel


class Piecewise:
    """fsets: (t, taps, onset or None), dsets: (t, delay), each ascending in t; mix(rows) is the next step, cut at `cuts` too"""

    def __init__(self, n_channels, n_obj, n_taps, max_onset, xfade, max_delay=None, ramp=0):
        self.delay = max_delay is not None
        self.model = (DelayModel(n_channels, n_obj, n_taps, max_onset, xfade, max_delay, ramp) if self.delay
                      else FirModel(n_channels, n_obj, n_taps, max_onset, xfade))
        self.t = 0
        self.fsets, self.dsets = [], []

    def schedule(self, times, taps, onsets=None):
        for k, t in enumerate(times):
            self.fsets.append((int(t), np.asarray(taps[k], dtype=np.float32), None if onsets is None else onsets[k]))

    def delay_schedule(self, times, delays):
        for k, t in enumerate(times):
            self.dsets.append((int(t), np.asarray(delays[k], dtype=np.float32)))

    def mix(self, rows, cuts=()):
        rows = np.asarray(rows, dtype=np.float32)
        n = rows.shape[1]
        t0, t1 = self.t, self.t + n
        assert all(t >= t0 for t, *_ in self.fsets + self.dsets)
        edges = sorted({t0, t1} | {t for t, *_ in self.fsets + self.dsets if t < t1} | {t0 + c for c in cuts if 0 < c < n})
        outs = []
        for a, b in zip(edges[:-1], edges[1:]):
            while self.fsets and self.fsets[0][0] == a:
                _, h, on = self.fsets.pop(0)
                self.model.set(h, on)
            while self.dsets and self.dsets[0][0] == a:
                self.model.set_delay(self.dsets.pop(0)[1])
            outs.append(self.model.mix(rows[:, a - t0:b - t0]))
        self.t = t1
        return np.concatenate(outs, axis=1)
