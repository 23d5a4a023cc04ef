"""Modulation maps (Engine.set_modulation / fetch_modulation): Schroeder's modulation transfer function per octave band and the speech
transmission index (STI, IEC 60268-16, indirect method) at every node of a box, from ONE run.

The engine keeps, per node and band k, the energy E[k] of the band-filtered captures and the Fourier sums of their SQUARES at M
modulation frequencies (include/wayverb_amd.h, "modulation maps").  modulation_fold is the DEFINITION of that fold, in NumPy, bit for
bit; mtf, transmission_index, mti and sti are what the standard makes of the sums.

What is left out: auditory masking and the reception threshold, which need absolute levels, and noise.  This is the level-independent
indirect method: STI from the impulse response alone."""
import numpy as np

from . import decay as _decay

# the standard's 14 modulation frequencies (Hz) and 7 octave bands (Hz)
STI_MODULATION_HZ = (0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5)
STI_OCTAVE_HZ = (125, 250, 500, 1000, 2000, 4000, 8000)
# male speech: band weights alpha and redundancy corrections beta between neighbouring bands; sum(alpha) - sum(beta) = 1
STI_ALPHA = (0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173)
STI_BETA = (0.085, 0.078, 0.065, 0.011, 0.047, 0.095)


def cycles_per_step(hz, sample_rate):
    """Modulation frequencies in hertz -> cycles per STEP of a mesh stepped at `sample_rate` (whatever the plan's period)."""
    return np.asarray(hz, dtype=np.float64) / float(sample_rate)


def modulation_fold(snaps, steps, freqs, sections, state=None, sums=None, return_state=False):
    """What a modulation plan folds, from the snapshots float32[n, ...nodes] of the same plan and their steps [n]: freqs float64[M] in
    cycles per step, sections float64[K][S][5] -> (energy float64[K, ...nodes], sums complex128[K, M, ...nodes]).  Per band the
    cascade of decay.biquad_cascade, then in capture order e = y * y, E = E + e, Re = Re + e * c, Im = Im - e * s with (c, s) =
    engine.spectrum_twiddle(f_m, step) -- every product and sum a float64 array operation of its own.  `state` float64[K][S][2,
    ...nodes] and `sums` = (energy, sums) continue an earlier call (neither is modified); return_state adds the final state."""
    from . import engine as E
    sections = np.asarray(sections, dtype=np.float64)
    sections = sections.reshape((-1,) + sections.shape[-2:])
    freqs = np.asarray(freqs, dtype=np.float64).reshape(-1)
    x = np.asarray(snaps).astype(np.float64)
    steps = [int(n) for n in np.asarray(steps).reshape(-1)]
    if len(steps) != x.shape[0]:
        raise ValueError("modulation_fold: one step per snapshot")
    n_bands, n_freqs, nodes = sections.shape[0], freqs.shape[0], x.shape[1:]
    if sums is None:
        energy, re, im = np.zeros((n_bands,) + nodes), np.zeros((n_bands, n_freqs) + nodes), np.zeros((n_bands, n_freqs) + nodes)
    else:
        energy = np.array(sums[0], dtype=np.float64).reshape((n_bands,) + nodes)
        acc = np.asarray(sums[1], dtype=np.complex128).reshape((n_bands, n_freqs) + nodes)
        re, im = acc.real.copy(), acc.imag.copy()
    twiddles = [[E.spectrum_twiddle(f, n) for f in freqs] for n in steps]
    states = []
    for k in range(n_bands):
        y, z = _decay.biquad_cascade(sections[k], x, None if state is None else state[k])
        states.append(z)
        for j in range(x.shape[0]):
            e = y[j] * y[j]
            energy[k] = energy[k] + e
            for m, (c, s) in enumerate(twiddles[j]):
                re[k, m] = re[k, m] + e * c
                im[k, m] = im[k, m] - e * s
    out = np.empty((n_bands, n_freqs) + nodes, dtype=np.complex128)
    out.real, out.imag = re, im
    return (energy, out, np.array(states)) if return_state else (energy, out)


def mtf(energy, sums):
    """The modulation transfer function m[K, M, ...nodes] = |sums| / energy; NaN where the energy is 0."""
    energy = np.asarray(energy, dtype=np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(energy == 0, np.nan, np.abs(np.asarray(sums)) / energy)


def transmission_index(m):
    """The standard's transmission index of a modulation transfer value: SNR = 10 log10(m / (1 - m)) clipped to -15 .. +15 dB,
    TI = (SNR + 15) / 30.  m >= 1 gives 1, m <= 0 gives 0, NaN stays NaN."""
    m = np.asarray(m, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = 10.0 * np.log10(m / (1.0 - m))
        ti = (np.clip(snr, -15.0, 15.0) + 15.0) / 30.0
    ti = np.where(m >= 1.0, 1.0, np.where(m <= 0.0, 0.0, ti))
    return np.where(np.isnan(m), np.nan, ti)


def mti(m, axis=1):
    """The modulation transfer index of every band: the mean transmission index over the modulation axis of m[K, M, ...nodes]."""
    return transmission_index(m).mean(axis=axis)


def sti(mti_by_band, rest=None):
    """STI = sum_k alpha_k MTI_k - sum_k beta_k sqrt(MTI_k MTI_k+1) over the seven octave bands 125 Hz .. 8 kHz, the standard's male
    weights.  `mti_by_band`: {octave centre in Hz: MTI scalar or map}; `rest`: the same for the octave bands the mesh does not carry
    (a waveguide is trusted up to about a quarter of its sample rate; the bands above come from a geometric method or a measurement),
    or one scalar for all of them.  A band found in neither raises ValueError naming it.  See the module's docstring for what is
    left out: masking, the reception threshold and noise."""
    given = {int(round(float(c))): np.asarray(v, dtype=np.float64) for c, v in dict(mti_by_band).items()}
    if rest is not None and not hasattr(rest, "items"):
        rest = {c: rest for c in STI_OCTAVE_HZ if c not in given}
    extra = {int(round(float(c))): np.asarray(v, dtype=np.float64) for c, v in dict(rest or {}).items()}
    bands = []
    for centre in STI_OCTAVE_HZ:
        if centre in given:
            bands.append(given[centre])
        elif centre in extra:
            bands.append(extra[centre])
        else:
            raise ValueError("sti: no modulation transfer index for the %d Hz octave band (mti_by_band and rest hold neither)" % centre)
    total = 0.0
    for a, v in zip(STI_ALPHA, bands):
        total = total + a * v
    for b, lo, hi in zip(STI_BETA, bands[:-1], bands[1:]):
        total = total - b * np.sqrt(lo * hi)
    return total


def schroeder_mtf(hz, t60):
    """Schroeder's closed form for an exponential decay of reverberation time t60 (s): 1 / sqrt(1 + (2 pi F t60 / 13.8155)^2)."""
    return 1.0 / np.sqrt(1.0 + (2.0 * np.pi * np.asarray(hz, dtype=np.float64) * float(t60) / 13.8155) ** 2)
