// Host walk of n3dt_mel_spectrogram's frames (tests/test_mel_cpu.py builds this with the host compiler and the address and
// undefined-behaviour sanitizers and runs it on a fixture waveform).  It includes the very header the kernel is compiled from,
// csrc/mel_core.h, and runs its phases in plain loops over `tid` where the kernel has one thread per tid and a barrier between
// phases -- so the reflection on either side, the pre-emphasis carry and every bound are exercised on the CPU before a GPU
// sees them.
//
// usage: mel_core_host FILE      FILE = int64 L; float32 wav[L]; float64 table[800]; float32 basis[80][401]
// prints one line per value:  <frame> <band> <value %.17g>
// Every frame that a run starting mid-signal can hold (the streaming form's call) is computed a second time from the shortest such
// run, copied into memory of exactly its size; a value that differs from the whole signal's by a single bit ends the program
// with status 3.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../nerf-3dtalker-code_amd/csrc/mel_core.h"

// the kernel's body for one frame; basis_t is the transposed basis the first launch leaves in the workspace
static void frame(MelFrameMem* m, const MelSignal* sig, long long t, const float* basis_t, double* out80) {
    for (int tid = 0; tid < MEL_THREADS; ++tid) mel_stage(m, tid, MEL_THREADS, sig, t);
    for (int tid = 0; tid <= MEL_HALF / 2; ++tid) mel_bin_pair(m, tid);
    for (int tid = 0; tid < MEL_NMELS; ++tid) out80[tid] = mel_normalise(mel_filter(m, tid, basis_t));
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s FILE\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    int64_t L = 0;
    if (std::fread(&L, sizeof(L), 1, f) != 1 || L < MEL_MIN_SAMPLES || L > (1 << 24)) return 2;
    // exactly the bytes the entry point is given: the sanitizer sees any read past the waveform, the table or the basis
    std::vector<float> wav((size_t)L), basis((size_t)MEL_NMELS * MEL_BINS), basis_t((size_t)MEL_BINS * MEL_NMELS);
    std::vector<double> table(MEL_NFFT);
    if (std::fread(wav.data(), sizeof(float), wav.size(), f) != wav.size()) return 2;
    if (std::fread(table.data(), sizeof(double), table.size(), f) != table.size()) return 2;
    if (std::fread(basis.data(), sizeof(float), basis.size(), f) != basis.size()) return 2;
    std::fclose(f);
    for (int o = 0; o < MEL_BINS * MEL_NMELS; ++o) basis_t[o] = basis[(o % MEL_NMELS) * MEL_BINS + o / MEL_NMELS];

    const long long T = mel_frames(L);
    auto m = std::make_unique<MelFrameMem>();  // one workgroup's LDS
    for (int tid = 0; tid < MEL_THREADS; ++tid) mel_load_table(m.get(), tid, MEL_THREADS, table.data());
    MelSignal whole = {wav.data(), nullptr, L, 0, L};
    if (mel_run_covers(L, 0, L, 0, 0, T)) return 2;
    std::vector<double> mel((size_t)T * MEL_NMELS);
    for (long long t = 0; t < T; ++t) frame(m.get(), &whole, t, basis_t.data(), &mel[(size_t)t * MEL_NMELS]);

    double again[MEL_NMELS];
    for (long long t = 3; t < T; ++t) {  // frames 0 .. 2 start at or before sample 0
        const long long hi = mel_frame_hi(t), mirrored = 2 * ((long long)L - 1) - hi;
        const bool tail = hi > L - 1;
        // an interior frame from a run whose end is unknown: exactly its 800 samples; a tail frame from a run that ends the signal
        // and starts at the first sample the frame or its reflection reads
        const long long lo = tail && mirrored < mel_frame_lo(t) ? mirrored : mel_frame_lo(t);
        const long long n = tail ? L - lo : MEL_NFFT;
        std::vector<float> run(wav.begin() + lo, wav.begin() + lo + n), prev(1, wav[lo - 1]);
        const long long total = tail ? (long long)L : -1;
        if (mel_run_covers(n, lo, total, 1, t, 1)) return 2;
        MelSignal sig = {run.data(), prev.data(), n, lo, total};
        frame(m.get(), &sig, t, basis_t.data(), again);
        if (std::memcmp(again, &mel[(size_t)t * MEL_NMELS], sizeof(again)) != 0) {
            std::fprintf(stderr, "frame %lld differs when computed from a run that starts at sample %lld\n", t, lo);
            return 3;
        }
    }
    // what the entry point must refuse: a run that starts after or ends before what the frames read, a missing carry
    if (!mel_run_covers(L - 1, 1, L, 1, 0, 1) || !mel_run_covers(L, 0, -1, 0, T - 1, 1) || !mel_run_covers(L - 200, 200, L, 0, 3, 1)) return 4;

    for (long long t = 0; t < T; ++t)
        for (int i = 0; i < MEL_NMELS; ++i) std::printf("%lld %d %.17g\n", t, i, mel[(size_t)t * MEL_NMELS + i]);
    return 0;
}
