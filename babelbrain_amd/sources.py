"""Separable (low-rank) source tables: the second, opt-in form of the solver's `PulseSource`.

Every transducer of the reference builds each PulseSource row as |u| sin(2 pi f t + arg u) ramp(t) (Single:341-342 and its
siblings), so every row is a fixed combination of two shared time signals:
    |u| cos(arg u) * sin(2 pi f t) ramp(t)  +  |u| sin(arg u) * cos(2 pi f t) ramp(t).
A `SeparableSource(weights, signals)` holds per-row weights [nSources][K] and shared signals [K][nT] in float32 and means
exactly this table ("Sources"):
    acc = w[r,0]*s[0,n]; acc = acc + w[r,1]*s[1,n]; ...
evaluated in float32, in that order, with no FMA contraction and float32 denormals flushed to zero -- what the device does
(bfd_set_sources_separable). `dense()` restates it on the host as the float64 [nSources][nT] table of those float32 values;
the dense path fed that table computes the same results bit for bit.
"""
import numpy as np

FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def _ftz(a):
    """Flush float32 denormals to (signed) zero, in place; returns a."""
    a[np.abs(a) < FLT_MIN] *= np.float32(0)
    return a


def _ramp(freq, dt, ramp_length):
    """The half-cosine ramp of the reference's source builders (Single:335-338, as in harness.pulse_sources)."""
    rp = int(np.round(ramp_length / freq / dt))
    return (-np.cos(np.arange(0, np.pi, np.pi / rp)) + 1) * 0.5


def cw_time(freq, dt, T):
    """Time vector of the reference's source builders: length = floor(T f) / f, tv = arange(0, length + dt, dt)."""
    length = np.floor(T / (1.0 / freq)) * 1 / freq
    return np.arange(0, length + dt, dt)


def cw_envelope(freq, dt, T, ramp_length=4, ramp_both_ends=False):
    """float64 envelope over cw_time(): the ramp at the start (and mirrored at the end with ramp_both_ends, CONCAVE:395-397)."""
    nT = cw_time(freq, dt, T).shape[0]
    ramp = _ramp(freq, dt, ramp_length)
    env = np.ones(nT)
    nr = min(len(ramp), nT)
    env[:nr] *= ramp[:nr]
    if ramp_both_ends:
        env[-len(ramp):] *= np.flip(ramp)[-nT:]
    return env


class SeparableSource:
    """PulseSource[r, n] = sum_k weights[r, k] * signals[k, n] in float32, in order k = 0, 1, ... (see the module docstring).
    weights: [nSources][K], signals: [K][nT], 1 <= K <= 4, finite; both are rounded once to float32 and their denormals
    flushed to zero."""

    def __init__(self, weights, signals):
        with np.errstate(over='ignore', invalid='ignore'):        # values beyond float32 become inf: rejected below
            w = np.array(weights, dtype=np.float32, copy=True)
            s = np.array(signals, dtype=np.float32, copy=True)
        if w.ndim != 2 or s.ndim != 2:
            raise ValueError('SeparableSource: weights must be [nSources][K] and signals [K][nT]')
        K = w.shape[1]
        if not 1 <= K <= 4:
            raise ValueError('SeparableSource: K must be 1..4, got %d' % K)
        if s.shape[0] != K:
            raise ValueError('SeparableSource: weights have K=%d columns but signals have %d rows' % (K, s.shape[0]))
        if not (np.all(np.isfinite(w)) and np.all(np.isfinite(s))):
            raise ValueError('SeparableSource: weights and signals must be finite (in float32)')
        self.weights = np.ascontiguousarray(_ftz(w))
        self.signals = np.ascontiguousarray(_ftz(s))

    @property
    def K(self):
        return self.weights.shape[1]

    @property
    def shape(self):
        """(nSources, nT), like the dense PulseSource table."""
        return (self.weights.shape[0], self.signals.shape[1])

    @property
    def nbytes(self):
        return self.weights.nbytes + self.signals.nbytes

    def dense(self):
        """The float64 [nSources][nT] table this object means: float32 products and sums in the stated order, each flushed."""
        w, s = self.weights, self.signals
        acc = _ftz(w[:, 0:1] * s[0:1, :])
        for k in range(1, self.K):
            acc = _ftz(acc + _ftz(w[:, k:k + 1] * s[k:k + 1, :]))
        return acc.astype(np.float64)

    def __repr__(self):
        return 'SeparableSource(nSources=%d, K=%d, nT=%d)' % (self.shape[0], self.K, self.shape[1])

    @classmethod
    def cw(cls, u_complex, freq, dt, T, ramp_length=4, ramp_both_ends=False):
        """Continuous-wave rows |u| sin(2 pi f t + arg u) env(t), one per element of u_complex (in its flat order), over the
        reference's time vector and half-cosine ramp: K = 2, weights [|u| cos arg u, |u| sin arg u], signals
        [sin(2 pi f t) env, cos(2 pi f t) env], computed in float64 and rounded once to float32."""
        u = np.asarray(u_complex).reshape(-1).astype(np.complex128)
        wt = 2 * np.pi * freq * cw_time(freq, dt, T)
        env = cw_envelope(freq, dt, T, ramp_length, ramp_both_ends)
        amp, ph = np.abs(u), np.angle(u)
        weights = np.stack([amp * np.cos(ph), amp * np.sin(ph)], axis=1)
        signals = np.stack([np.sin(wt) * env, np.cos(wt) * env], axis=0)
        return cls(weights, signals)
