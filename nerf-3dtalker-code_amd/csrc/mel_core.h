/*
 * mel_core.h -- the per-frame arithmetic of n3dt_mel_spectrogram (include/n3dt.h): a 16 kHz waveform to the normalised
 * 80-band mel spectrogram that Audio2style was trained on (the reference's wav_audio.melspectrogram with wav_hparams.py;
 * DESIGN section 3.15 holds the formulation).  Everything is float64.
 *
 * Included by csrc/mel.hip, whose kernel runs the phases below with one thread per `tid` and a workgroup barrier between two
 * phases, and by tests/mel_core_host.cpp, which runs the very same functions in plain loops on the CPU (under the address and
 * undefined-behaviour sanitizers), so the reflection, carry and bounds logic is checked without a GPU.  Compiles as host C++ on
 * its own; the __host__ __device__ qualifiers exist only under hipcc.
 *
 * One workgroup owns one frame t at a time:
 *   mel_load_table  the 800-entry cosine table into MelFrameMem (once per workgroup);
 *   mel_stage       the frame's 800 windowed samples, folded: pre-emphasis and reflect padding happen in the fetch (mel_sample),
 *                   by signal index, so no padded or filtered copy of the waveform exists anywhere.  A real frame's twiddles
 *                   repeat, cos(k (800 - n)) = cos(k n) and sin(k (800 - n)) = -sin(k n), so the sums run over n = 0 .. 399 of
 *                   e[n] = ws[n] + ws[800 - n] against the cosine and o[n] = ws[n] - ws[800 - n] against the sine (e[0] = ws[0],
 *                   o[0] = 0; ws[400] meets cos(k pi) = +-1 alone);
 *   mel_bin_pair    |D[k]| and |D[400 - k]| of one k <= 200: cos((400 - k) n) = (-1)^n cos(k n) and likewise for the sine, so the
 *                   even and the odd n are added in separate chains (200 fused multiply-adds each, in the order of n) and the two
 *                   bins are their sum and their difference; twiddles from the table at (k n) mod 800, sine a quarter turn back;
 *   mel_filter      one row of basis . |D|, 401 fused multiply-adds in the order k = 0 .. 400;
 *   mel_normalise   amplitude -> dB -> [-4, 4].
 * A frame's value is a function of (the samples it touches, table, basis) alone: nothing depends on the grid, on the frame's
 * position in the call or on how many frames the call computes.  The streaming form relies on that bit for bit.
 */
#ifndef N3DT_MEL_CORE_H
#define N3DT_MEL_CORE_H

#include <math.h>

#ifdef __HIPCC__
#define MEL_HD __host__ __device__ static inline
#else
#define MEL_HD static inline
#endif

/* wav_hparams.py */
#define MEL_SAMPLE_RATE 16000
#define MEL_NFFT 800                 /* n_fft == win_size */
#define MEL_HOP 200
#define MEL_NMELS 80
#define MEL_FMIN 55.0
#define MEL_FMAX 7600.0
#define MEL_PREEMPHASIS 0.97
#define MEL_MIN_LEVEL_DB (-100.0)
#define MEL_REF_LEVEL_DB 20.0
#define MEL_MAX_ABS_VALUE 4.0        /* symmetric, clipped */

#define MEL_PAD (MEL_NFFT / 2)       /* reflect padding on either side */
#define MEL_BINS (MEL_NFFT / 2 + 1)  /* 401 */
#define MEL_MIN_SAMPLES (MEL_PAD + 1) /* a reflection of 400 needs 401 samples */
#define MEL_QUARTER (MEL_NFFT / 4)
#define MEL_AMP_FLOOR 1e-5           /* 10 ^ (min_level_db / 20) */
#define MEL_WINDOW_COLS 16           /* columns of one Audio2style window */
#define MEL_HALF (MEL_NFFT / 2)
#define MEL_THREADS 256              /* four waves: 201 bin pairs */
#define MEL_MAX_FRAMES (1 << 24)     /* per call (more than two days of audio) */

/* A run of the signal: wav[0 .. n_samples) are the samples offset .. offset + n_samples of a signal of `total` samples
 * (total < 0: the end is not known yet, nothing is reflected on the right).  prev is the sample offset - 1 (read only when
 * offset > 0). */
typedef struct MelSignal {
    const float* wav;
    const float* prev;
    long long n_samples, offset, total;
} MelSignal;

typedef struct MelFrameMem {
    double tab[MEL_NFFT];  /* cos(2 pi n / 800) */
    double eo[MEL_HALF][2]; /* {e[n], o[n]} of the windowed, pre-emphasised, padded frame */
    double mid;            /* its sample 400 */
    double mag[MEL_BINS];
} MelFrameMem;

/* number of frames of a signal of L samples */
MEL_HD long long mel_frames(long long L) { return 1 + L / MEL_HOP; }

/* the first and the last signal index frame t reads, before reflection */
MEL_HD long long mel_frame_lo(long long t) { return t * MEL_HOP - MEL_PAD; }
MEL_HD long long mel_frame_hi(long long t) { return t * MEL_HOP - MEL_PAD + MEL_NFFT - 1; }

/* NULL when the run holds every sample the frames first .. first + n - 1 read, else what is missing.  The kernel indexes wav
 * with nothing but what this accepts. */
MEL_HD const char* mel_run_covers(long long n_samples, long long offset, long long total, int have_prev, long long first, long long n) {
    if (n_samples < 1 || offset < 0 || first < 0 || n < 1) return "n_samples, n_frames must be >= 1 and wav_offset, first_frame >= 0";
    const long long end = offset + n_samples;  /* one past the last sample held */
    if (offset > 0 && !have_prev) return "prev_sample is NULL but wav_offset > 0";
    if (total >= 0) {
        if (total < MEL_MIN_SAMPLES) return "the signal must have at least 401 samples";
        if (end != total) return "total_samples given: the run must end at the signal's end";
        if (first + n > mel_frames(total)) return "frames past 1 + total_samples / 200";
    }
    long long lo = mel_frame_lo(first), hi = mel_frame_hi(first + n - 1);
    if (lo < 0) {  /* reflected about sample 0: indices 0 .. 400 */
        if (offset != 0) return "the first frames reflect about sample 0: the run must start there";
        if (end < MEL_MIN_SAMPLES) return "the left reflection needs 401 samples";
        lo = 0;
    }
    if (total >= 0 && hi > total - 1) {  /* reflected about the last sample: down to 2 (total - 1) - hi >= total - 401 */
        const long long r = 2 * (total - 1) - hi;
        if (r < lo) lo = r;
        hi = total - 1;
    }
    if (lo < offset) return "the run starts after the first sample the frames read";
    if (hi >= end) return "the run ends before the last sample the frames read";
    return 0;
}

/* pre-emphasised sample s of the reflect-padded signal, s in [-400, total + 400) */
MEL_HD double mel_sample(const MelSignal* g, long long s) {
    if (s < 0) s = -s;
    if (g->total >= 0 && s > g->total - 1) s = 2 * (g->total - 1) - s;
    const long long i = s - g->offset;
    const double x = (double)g->wav[i];
    if (s == 0) return x;
    const double xp = (double)(i > 0 ? g->wav[i - 1] : g->prev[0]);
    return x - MEL_PREEMPHASIS * xp;
}

MEL_HD void mel_load_table(MelFrameMem* m, int tid, int nthreads, const double* table) {
    for (int n = tid; n < MEL_NFFT; n += nthreads) m->tab[n] = table[n];
}

/* needs mel_load_table (and a barrier) first: the periodic Hann window is 0.5 - 0.5 cos(2 pi n / 800), the same at n and 800 - n */
MEL_HD void mel_stage(MelFrameMem* m, int tid, int nthreads, const MelSignal* g, long long t) {
    const long long s0 = mel_frame_lo(t);
    for (int n = tid; n <= MEL_HALF; n += nthreads) {
        const double w = 0.5 - 0.5 * m->tab[n];
        const double a = w * mel_sample(g, s0 + n);
        if (n == MEL_HALF) {
            m->mid = a;
        } else if (n == 0) {
            m->eo[0][0] = a;
            m->eo[0][1] = 0.0;
        } else {
            const double b = w * mel_sample(g, s0 + MEL_NFFT - n);
            m->eo[n][0] = a + b;
            m->eo[n][1] = a - b;
        }
    }
}

/* the table's entry a quarter turn back: sin(2 pi i / 800) */
MEL_HD double mel_sine(const MelFrameMem* m, int idx) {
    return m->tab[idx >= MEL_QUARTER ? idx - MEL_QUARTER : idx + (MEL_NFFT - MEL_QUARTER)];
}

/* k in 0 .. 200: mag[k] and (k < 200) mag[400 - k] */
MEL_HD void mel_bin_pair(MelFrameMem* m, int k) {
    double ce = 0.0, co = 0.0, se = 0.0, so = 0.0;  /* cosine and sine sums over the even and over the odd n */
    int idx = 0;                                    /* (k n) mod 800 */
    for (int n = 0; n < MEL_HALF; n += 2) {
        ce = fma(m->eo[n][0], m->tab[idx], ce);
        se = fma(m->eo[n][1], mel_sine(m, idx), se);
        idx += k;
        if (idx >= MEL_NFFT) idx -= MEL_NFFT;
        co = fma(m->eo[n + 1][0], m->tab[idx], co);
        so = fma(m->eo[n + 1][1], mel_sine(m, idx), so);
        idx += k;
        if (idx >= MEL_NFFT) idx -= MEL_NFFT;
    }
    const double mid = (k & 1) ? -m->mid : m->mid;  /* n = 400: cos(k pi); 400 - k has k's parity */
    double re = (ce + co) + mid, im = se + so;
    m->mag[k] = sqrt(re * re + im * im);
    if (k < MEL_HALF / 2) {
        re = (ce - co) + mid;
        im = se - so;
        m->mag[MEL_HALF - k] = sqrt(re * re + im * im);
    }
}

/* basis_t: the fp32 basis transposed, [401][80] */
MEL_HD double mel_filter(const MelFrameMem* m, int i, const float* basis_t) {
    double acc = 0.0;
    for (int k = 0; k < MEL_BINS; ++k) acc = fma((double)basis_t[k * MEL_NMELS + i], m->mag[k], acc);
    return acc;
}

/* NaN stays NaN through the floor and the clip, as numpy.maximum and numpy.clip keep it */
MEL_HD double mel_normalise(double amp) {
    const double a = !(amp <= MEL_AMP_FLOOR) ? amp : MEL_AMP_FLOOR;
    const double db = 20.0 * log10(a) - MEL_REF_LEVEL_DB;
    const double v = (2.0 * MEL_MAX_ABS_VALUE) * ((db - MEL_MIN_LEVEL_DB) / (-MEL_MIN_LEVEL_DB)) - MEL_MAX_ABS_VALUE;
    return v < -MEL_MAX_ABS_VALUE ? -MEL_MAX_ABS_VALUE : (v > MEL_MAX_ABS_VALUE ? MEL_MAX_ABS_VALUE : v);
}

/* column of window w's c-th entry, clamped into the spectrogram */
MEL_HD long long mel_window_col(int start, int c, long long T) {
    const long long j = (long long)start + c;
    return j < 0 ? 0 : (j > T - 1 ? T - 1 : j);
}

#endif
