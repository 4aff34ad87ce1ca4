// The audio front end (include/n3dt.h, n3dt_mel_spectrogram / n3dt_mel_windows): a 16 kHz waveform to the normalised mel
// windows Audio2style reads, as the reference's wav_audio.melspectrogram and its data loader produce them on the CPU.  The
// arithmetic lives in mel_core.h, which a host program also compiles; this file is the kernels that run it.
//
// Data path: wav fp32 -> (mel_spectrogram_kernel) mel [80, T] float64 or fp32 -> (mel_windows_kernel) [N, 80, 16] fp32.
//
// mel_basis_transpose_kernel: the caller's basis [80, 401] -> workspace [401, 80], so that the 80 threads of the filter phase
// read consecutive floats.  32 080 elements; it runs in front of every spectrogram call because the basis is the caller's memory.
//
// mel_spectrogram_kernel: one workgroup of 256 threads (four waves) per frame, grid-stride over the call's frames.  Pre-emphasis,
// reflect padding and the window are applied while the 800 samples are fetched and folded into LDS (a real frame's twiddles
// repeat: 400 terms per sum, not 800); thread k <= 200 then owns the bins k and 400 - k, which share their twiddles up to a sign,
// and adds their terms with v_fma_f64 in the order of n, reading the twiddles from the 800-entry cosine table in LDS at
// (k n) mod 800; thread i < 80 adds filter i's 401 terms in bin order, normalises and stores one value.  16 KiB of LDS, no
// atomics, no intermediate in HBM.  The loop is bound by its LDS reads (two gathered twiddles and one broadcast pair of samples
// per two multiply-adds; more accumulator chains changed nothing), which is why the fold and the bin pairing pay: 3.5 x fewer
// reads than one thread per bin over 800 terms.  Plain FMA rather than v_mfma_f64_16x16x4_f64: a 16-frame x 16-bin MFMA tile
// would need its B operand (the twiddles of 16 bins x 4 samples) gathered from the table for every step, which costs the LDS
// reads the FMA form already pays, and one second of audio is 81 frames -- 6 such tiles would leave 250 CUs idle where 81
// workgroups do not.
//
// mel_windows_kernel: one thread per output value; column indices are clamped into [0, T - 1].
#include <hip/hip_runtime.h>

#include "mel_core.h"
#include "n3dt_launch.h"

#define MEL_MAX_GRID 65536

__global__ __launch_bounds__(256) void mel_basis_transpose_kernel(const float* __restrict__ basis, float* __restrict__ basis_t) {
    const int o = (int)(blockIdx.x * blockDim.x + threadIdx.x);  // index into [401][80]
    if (o < MEL_BINS * MEL_NMELS) {
        const int k = o / MEL_NMELS, i = o - k * MEL_NMELS;
        basis_t[o] = basis[i * MEL_BINS + k];
    }
}

__global__ __launch_bounds__(MEL_THREADS) void mel_spectrogram_kernel(MelSignal sig, long long first_frame, int n_frames,
                                                                      const float* __restrict__ basis_t, const double* __restrict__ table,
                                                                      void* __restrict__ out, long long out_ld, int out_is_f64) {
    __shared__ MelFrameMem m;
    const int tid = (int)threadIdx.x;
    mel_load_table(&m, tid, MEL_THREADS, table);
    __syncthreads();
    for (int f = (int)blockIdx.x; f < n_frames; f += (int)gridDim.x) {
        mel_stage(&m, tid, MEL_THREADS, &sig, first_frame + f);
        __syncthreads();
        if (tid <= MEL_HALF / 2) mel_bin_pair(&m, tid);
        __syncthreads();
        if (tid < MEL_NMELS) {
            const double v = mel_normalise(mel_filter(&m, tid, basis_t));
            const long long o = (long long)tid * out_ld + f;
            if (out_is_f64) ((double*)out)[o] = v;
            else ((float*)out)[o] = (float)v;
        }
        // m.eo and m.mag are written again only after the next frame's barriers: the filter phase reads m.mag alone, and the next
        // mel_stage writes m.eo and m.mid alone, which no thread reads after the barrier above
    }
}

__global__ __launch_bounds__(256) void mel_windows_kernel(const void* __restrict__ mel, long long T, long long mel_ld, int mel_is_f64,
                                                          const int* __restrict__ start, long long total, float* __restrict__ out) {
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
        const long long w = o / (MEL_NMELS * MEL_WINDOW_COLS);
        const int r = (int)(o - w * (MEL_NMELS * MEL_WINDOW_COLS));
        const int i = r / MEL_WINDOW_COLS, c = r - i * MEL_WINDOW_COLS;
        const long long src = (long long)i * mel_ld + mel_window_col(start[w], c, T);
        out[o] = mel_is_f64 ? (float)((const double*)mel)[src] : ((const float*)mel)[src];
    }
}

extern "C" size_t n3dt_mel_ws_bytes(void) { return (size_t)MEL_BINS * MEL_NMELS * sizeof(float); }

extern "C" void n3dt_launch_mel_spectrogram(const MelSignal* sig, long long first_frame, int n_frames, const float* basis,
                                            const double* table, void* out, long long out_ld, int out_is_f64, void* workspace,
                                            hipStream_t stream) {
    float* basis_t = (float*)workspace;
    hipLaunchKernelGGL(mel_basis_transpose_kernel, dim3((MEL_BINS * MEL_NMELS + 255) / 256), dim3(256), 0, stream, basis, basis_t);
    hipLaunchKernelGGL(mel_spectrogram_kernel, dim3(n_frames < MEL_MAX_GRID ? n_frames : MEL_MAX_GRID), dim3(MEL_THREADS), 0, stream,
                       *sig, first_frame, n_frames, (const float*)basis_t, table, out, out_ld, out_is_f64);
}

extern "C" void n3dt_launch_mel_windows(const void* mel, long long T, long long mel_ld, int mel_is_f64, const int* start, int n_windows,
                                        float* out, hipStream_t stream) {
    const long long total = (long long)n_windows * MEL_NMELS * MEL_WINDOW_COLS;
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(mel_windows_kernel, dim3((unsigned)(blocks < MEL_MAX_GRID ? blocks : MEL_MAX_GRID)), dim3(256), 0, stream, mel, T,
                       mel_ld, mel_is_f64, start, total, out);
}
