"""The reference of the scene mix's schedule (include/openpbso_amd.h "The scene mix's SCHEDULE"): Model of tests/scene_mix_model.py
extended by sets that take effect at absolute samples.  A step is evaluated run by run -- the samples between two sets that fall
into it -- each run with the records in force there, through the unchanged evaluate() / tests/cpp/scene_mix_ref.c; a set is the
unchanged Model.set made at its own sample.  tests/test_scene_mix_sched_model.py anchors it on Model fed rows cut at every set."""
import numpy as np

from tests.scene_mix_model import Model, evaluate


class SchedModel(Model):
    def __init__(self, n_channels, n_obj, max_delay, ramp):
        super().__init__(n_channels, n_obj, max_delay, ramp)
        self.pending = []                                            # (t_set, gain, delay or None), ascending, none before self.t

    def set(self, gain, delay=None):
        assert not self.pending, "a plain set while scheduled sets are pending is refused"
        super().set(gain, delay)

    def set_at(self, t_set, gain, delay=None):
        assert t_set >= self.t and (not self.pending or t_set > self.pending[-1][0])
        g = np.array(gain, dtype=np.float32).reshape(self.C, self.N)
        d = None if delay is None else np.array(delay, dtype=np.float32).reshape(self.C, self.N)
        self.pending.append((int(t_set), g, d))

    def schedule(self, t_set, gain, delay=None):
        for k, t in enumerate(t_set):
            self.set_at(t, gain[k], None if delay is None else delay[k])

    def clear_schedule(self):
        self.pending = []

    def reset(self):
        super().reset()
        self.pending = []

    def mix(self, rows, samples=None):
        """rows [N][n] float32, the next step -> out [C][len(samples)] at the step's local samples (default: all of them)"""
        rows = np.asarray(rows, dtype=np.float32)
        n = rows.shape[1]
        samples = np.arange(n) if samples is None else np.asarray(samples, dtype=np.int64)
        t0 = self.t
        xx = np.concatenate([self.tail, rows], axis=1)               # xx[:, H + j] = x(t0 + j)
        inside = [q for q in self.pending if q[0] < t0 + n]
        self.pending = self.pending[len(inside):]
        out = np.zeros((self.C, samples.size), dtype=np.float32)
        edges = [t0] + [q[0] for q in inside] + [t0 + n]
        for k in range(len(edges) - 1):
            if k > 0:                                                # the set that begins this run, made at its own sample
                self.t = edges[k]
                Model.set(self, inside[k - 1][1], inside[k - 1][2])
            pick = np.flatnonzero((t0 + samples >= edges[k]) & (t0 + samples < edges[k + 1]))
            if pick.size:
                out[:, pick] = evaluate(xx, t0 - self.H, self.p, self.R, t0 + samples[pick])
        self.tail = np.ascontiguousarray(xx[:, xx.shape[1] - self.H:])
        self.t = t0 + n
        return out
