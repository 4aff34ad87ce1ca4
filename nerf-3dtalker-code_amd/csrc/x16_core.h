// Shared machinery of the 16-bit MFMA kernels (fused render forward, fused training forward / backward):
// fragment traits, the LDS weight stream, the fast positional encoding and small compile-time helpers.
#pragma once
#include <stdlib.h>

#include <type_traits>

#include "n3dt_device.h"
#include "n3dt_layout.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 x16_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 x16_f16x2 __attribute__((ext_vector_type(2)));
typedef float x16_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned x16_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned x16_u32x4 __attribute__((ext_vector_type(4)));

#define X16_BS 32
#define X16_CH 24                      // pieces per chunk (24 KiB)
#define X16_PIECE 1024                 // bytes
#define X16_NCHUNK (2280 / X16_CH)     // 48 + 6*288 + 336 + 24 + 144 pieces (RGB_layer_0 is merged into RGB_layer_1)
#define X16_XT_TILES 98                // saved activation tiles per block (training): PE 2 + 8 hidden layers x 12
#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

// Two floats -> one dword of two 16-bit values (a in the low half), round to nearest even: ONE v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32
// with both sources live.  Element-wise casts ((__bf16)v[j] in a loop, or an 8-wide __builtin_convertvector) are scalarised by
// hipcc into one conversion per VALUE -- the packed instruction with a dead second source, or v_cvt_f16_f32 -- plus a v_perm_b32 /
// v_pack_b32_f16 per dword to glue the halves together: 24 VALU instructions per 8-value fragment where 4 suffice.  The 2-wide
// vector conversion is the form it keeps whole.  Same rounding instruction, so every value converts to the same bits.
template <int PREC>
__device__ __forceinline__ unsigned x16_cvt2(const float a, const float b) {
    const x16_f32x2 p = {a, b};
    if constexpr (PREC == N3DT_BF16)
        return __builtin_bit_cast(unsigned, __builtin_convertvector(p, x16_bf16x2));
    else
        return __builtin_bit_cast(unsigned, __builtin_convertvector(p, x16_f16x2));
}
// eight floats -> one fragment, element j = v[j]
template <int PREC, class FRAG>
__device__ __forceinline__ FRAG x16_pack8(const float* v) {
    x16_u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = x16_cvt2<PREC>(v[2 * j], v[2 * j + 1]);
    return __builtin_bit_cast(FRAG, w);
}

template <int PREC>
struct X16;
template <>
struct X16<N3DT_BF16> {
    typedef bf16x8 frag;
    static __device__ __forceinline__ f32x16 mfma(frag a, frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ frag pack(const float* v) { return x16_pack8<N3DT_BF16, frag>(v); }
    // ReLU on the packed 16-bit values: a signed 16-bit max with 0 (v_pk_max_i16) clears exactly
    // the negative floats, and rounding commutes with it
    // `lo` = 0: ReLU;  lo = -32768 (the most negative 16-bit pattern): identity -- lets one rolled loop body serve
    // both the ReLU layers and the linear RGB_layer_0
    static __device__ __forceinline__ frag relu(frag f, short lo) {
        s16x8 s = __builtin_bit_cast(s16x8, f);
        s = __builtin_elementwise_max(s, (s16x8)(lo));
        return __builtin_bit_cast(frag, s);
    }
    // bias as an MFMA: A = [b_hi, b_lo, 0...] on the k = 0, 1 slots (lanes of the lower half), B = [1, 1, 0...]
    static __device__ __forceinline__ frag bias_frag(float b, bool lower_half) {
        __bf16 hi = (__bf16)b;
        __bf16 lo = (__bf16)(b - (float)hi);
        frag f;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (__bf16)0.0f;
        if (lower_half) {
            f[0] = hi;
            f[1] = lo;
        }
        return f;
    }
    static __device__ __forceinline__ frag ones_frag() {
        frag f;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (__bf16)(j < 2 ? 1.0f : 0.0f);
        return f;
    }
};
template <>
struct X16<N3DT_F16> {
    typedef f16x8 frag;
    static __device__ __forceinline__ f32x16 mfma(frag a, frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ frag pack(const float* v) { return x16_pack8<N3DT_F16, frag>(v); }
    // `lo` = 0: ReLU;  lo = -32768 (the most negative 16-bit pattern): identity -- lets one rolled loop body serve
    // both the ReLU layers and the linear RGB_layer_0
    static __device__ __forceinline__ frag relu(frag f, short lo) {
        s16x8 s = __builtin_bit_cast(s16x8, f);
        s = __builtin_elementwise_max(s, (s16x8)(lo));
        return __builtin_bit_cast(frag, s);
    }
    static __device__ __forceinline__ frag bias_frag(float b, bool lower_half) {
        _Float16 hi = (_Float16)b;
        _Float16 lo = (_Float16)(b - (float)hi);
        frag f;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (_Float16)0.0f;
        if (lower_half) {
            f[0] = hi;
            f[1] = lo;
        }
        return f;
    }
    static __device__ __forceinline__ frag ones_frag() {
        frag f;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (_Float16)(j < 2 ? 1.0f : 0.0f);
        return f;
    }
};

// The weight stream: X16_NCHUNK chunks of X16_CH pieces, staged L2 -> LDS by LDS-DMA into a ring of three
// chunk buffers (chunk c lives in buffer c % 3), and read by every wave through a small register ring of
// X16_DEPTH fragments so that the matrix pipe never waits for an LDS round trip:
//   * the prologue stages chunks 0 and 1 and meets once;
//   * rendezvous n (one workgroup barrier) is met X16_DEPTH pieces BEFORE the end of chunk n: it makes chunk
//     n+1 visible (issued after rendezvous n-1) and frees the buffer of chunk n-1, which every wave has left by
//     then, for chunk n+2 -- so fragment prefetches run across chunk boundaries without a bubble; chunk n+2 is
//     issued behind the barrier or spread over the pieces up to rendezvous n+1 (X16Issue below);
//   (a half-chunk stagger of the SIMD partner waves and an epilogue deferred onto a second accumulator set were
//   measured perf-neutral or worse in round 1 -- DESIGN 3.1 log items 3, 8, 11 -- and are gone from the source.)
#ifndef X16_DEPTH
#define X16_DEPTH 3  // fragments in flight per wave: 3 measured 0.6 % faster than 2 for the render kernel (same box), 4 spills it
#endif
#ifndef X16_NBUF
#define X16_NBUF 3  // chunk buffers of the ring (4 measured no faster for the render kernel and the renderer blocks)
#endif
#define X16_CHUNK_BYTES (X16_CH * X16_PIECE)

// WHERE a chunk's LDS-DMA pieces are issued: a compile-time schedule, template argument of WeightStream.
//   X16Issue<>             every piece right behind the rendezvous barrier, at piece X16_CH - DEPTH, each addressed through a
//                          per-lane 64-bit pointer: the form every kernel had, and the one the kernels without an A/B of their
//                          own keep (that path is the code it was);
//   X16Issue<S0, S1, ..>   piece i of the chunk a wave stages is issued by next<P>() when P % X16_CH == Si: PPW positions after
//                          the rendezvous piece and before the next one, i.e. from X16_CH - DEPTH + 1 .. X16_CH - 1, 0 ..
//                          X16_CH - DEPTH - 1, given in that order, so that the DMA instructions sit between MFMAs and not, all
//                          waves at once, beside the barrier wait, the matrix pipe's drain and a tile's epilogue.  The pieces are
//                          addressed from a scalar base (WeightStream::gsrc, voff).
// Invariants (WeightStream keeps them for every schedule; tests/test_host_stream_issue.py reads them off the assembly):
//   1. every piece of chunk c is issued, in program order, AFTER the rendezvous that frees the buffer of chunk c - NBUF (the one
//      met in chunk c - NBUF + 1) and BEFORE the next rendezvous, whose counted wait is the first that may have to cover it;
//   2. the tail of the stream (meets + NBUF - 1 >= limit) issues nothing;
//   3. the prologue stages its NBUF - 1 chunks whole, whatever the schedule;
//   4. the slots are positions P % X16_CH, so stages whose tiles are not one chunk (KS = 4, KS = 28) need no special case.
template <int... S>
struct X16Issue {
    static constexpr int count = sizeof...(S);
    static constexpr int at(const int i) {
        const int v[] = {S..., 0};
        return v[i];
    }
};

// Diagnostic build only (-DX16_STAMP): per-wave cycle sums of the three phases of a tile, written to the
// `wlocal` debug buffer (never read by the library).  Not for timing the kernel: the stamps fence overlap.
#ifdef X16_STAMP
__device__ __forceinline__ unsigned long long x16_now() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define X16_T(x) x
#else
#define X16_T(x)
#endif

// compile-time loop: f(std::integral_constant<int, I>) for I in [0, N) -- the piece index has to reach the
// inline-asm immediates as a constant expression
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// Keeping scalar loads out of the stream.  The counted fragment waits (s_waitcnt lgkmcnt(DEPTH-1)) share their counter
// with scalar memory loads, which return out of order.  That cannot make a wait pass EARLY -- the awaited fragment is the
// oldest LDS operation in flight and LDS returns in order, so while it is outstanding the younger prefetch behind it is
// too and the counter stays above DEPTH-1 whatever the scalar loads do -- but every stray s_load makes the wait longer
// (it has to drain as well) and costs an issue slot in the MFMA stream.  hipcc fetches kernel arguments lazily, at their
// first use, which can be deep inside the stream (seen: the output pointer of the fused renderer block, two arguments of
// the camera-gradient backward kernel).  Such kernels pass what they need later through x16_pin() before
// WeightStream::prologue_wait(): the empty asm forces the load up there and its opaque result cannot be re-fetched from
// the argument segment.  tools/check_smem_hazard.py scans the generated code for scalar / flat accesses inside streams.
// (pointers travel through the asm as integers and come back as global-address-space pointers: an opaque generic
// pointer would turn every access through it into a flat_ instruction, which counts on BOTH wait counters)
template <class T>
__device__ __forceinline__ void x16_pin(T& v) {
    static_assert(sizeof(T) <= 8, "scalar register pair at most");
    asm volatile("" : "+s"(v));
}
template <class T>
__device__ __forceinline__ void x16_pin(T*& p) {
    unsigned long long v = (unsigned long long)p;
    asm volatile("" : "+s"(v));
    p = (T*)(GLOBAL_AS T*)v;
}
template <class T>
__device__ __forceinline__ void x16_pin_v(T*& p) {  // per-lane pointers
    unsigned long long v = (unsigned long long)p;
    asm volatile("" : "+v"(v));
    p = (T*)(GLOBAL_AS T*)v;
}

#ifndef X16_RV_RAW
#define X16_RV_RAW 0
#endif
#ifndef X16_NT_STORE
#define X16_NT_STORE 1  // saved tiles are streamed (written once, read by a later kernel): nontemporal stores (fwd 1.65 -> 1.35 ms)
#endif
// DEPTH: fragments in flight per wave (DEPTH; the training forward runs with 2 to stay inside its register budget)
template <int PREC, int WAVES, int NCHUNK = X16_NCHUNK, int NBUF = X16_NBUF, int DEPTH = X16_DEPTH, class SCHED = X16Issue<>>
struct WeightStream {
    X16_T(unsigned long long t_rv = 0; unsigned long long t_mfma = 0; unsigned long long t_epi = 0; unsigned long long t_bias = 0;
          int tile_no = 0; float* tl = nullptr;)
    typedef typename X16<PREC>::frag frag;
    // Source of this wave's first piece: packed + (wave*PPW)*1KiB + lane*16.  X16Issue<>: gsrc is that per-lane pointer.  A spread
    // schedule: gsrc is its wave-uniform part and voff = lane*16, and a piece addresses as a scalar base (advanced by scalar
    // arithmetic) plus that one persistent 32-bit register, `global_load_lds_dwordx4 v, s[n:n+1]`, with no 64-bit vector add and
    // no register pair per piece.
    const unsigned char* gsrc;
    unsigned voff;
    unsigned char* ring;        // LDS, 3 chunk buffers
    unsigned lds_addr0;         // LDS byte address of ring + lane*16
    unsigned cur_addr, nxt_addr;  // LDS byte addresses (+ lane*16) of the buffers of chunk `chunk` and `chunk`+1
    int chunk;                  // chunk of the piece being consumed
    int meets;                  // rendezvous done so far
    int wave;
    // The stream can wrap around (prologue_issue(passes)): a persistent workgroup that walks several tiles keeps it running
    // across them.  Tried for the render kernel and not kept: with the tile body inlined into a tile loop hipcc hoists the
    // encoder's per-lane selectors and address constants out of the loop and spills (140 SGPR + 80 VGPR: 11.5 ms against
    // 7.2); with the body as a noinline callee (uniform arguments moved to SGPRs on entry) it still spills 15 fragments
    // (9.8 ms) -- the one-tile kernel sits at 254 of 256 registers and the loop adds a handful.  Results were correct.
    int limit;                  // chunks to stage in all: passes * NCHUNK
    int src_c;                  // source chunk of the next issue (wraps at NCHUNK: every pass streams the same weights)
    frag a[DEPTH];          // piece p sits in a[p % DEPTH]
    static constexpr int PPW = X16_CH / WAVES;  // pieces each wave stages per chunk
    // the issue schedule (X16Issue above)
    static constexpr bool SPREAD = SCHED::count != 0;
    static constexpr int RV = X16_CH - DEPTH;  // piece of a chunk at which the rendezvous is met
    static constexpr bool slots_in_order() {  // each in RV + 1 .. X16_CH - 1, 0 .. RV - 1, and in that order
        for (int i = 0; i < SCHED::count; ++i) {
            const int s = SCHED::at(i), prev = i ? SCHED::at(i - 1) : RV + 1;
            if (s < 0 || s >= X16_CH || s == RV || (s + X16_CH - RV - 1) % X16_CH < (prev + X16_CH - RV - 1) % X16_CH) return false;
        }
        return true;
    }
    static_assert(!SPREAD || SCHED::count == PPW, "one slot per piece a wave stages");
    static_assert(slots_in_order(), "slots lie between two rendezvous and are given in the order the stream passes them");
    int stage_c = -1;           // spread schedule: chunk (count since the prologue) whose pieces the slots are issuing; -1: none
    int stage_src;              // its source chunk

    __device__ __forceinline__ void issue(int c) {  // c: chunk count since the prologue (picks the ring buffer)
        if constexpr (SPREAD) {
            stage(c);
            static_for<0, PPW>([&](auto i_c) { issue_piece<decltype(i_c)::value>(); });
            stage_c = -1;
        } else {
            const unsigned char* src = gsrc + (size_t)src_c * X16_CHUNK_BYTES;
            src_c = src_c + 1 == NCHUNK ? 0 : src_c + 1;
            unsigned char* dst = ring + (c % NBUF) * X16_CHUNK_BYTES + wave * PPW * X16_PIECE;
            // (the instruction's immediate offset is not used: with one M0 and offsets 0 / 1 KiB / 2 KiB, and with a per-piece
            // M0 plus the offset on top, the fused kernel's results were wrong -- its effect on the LDS address was not pinned down)
#pragma unroll
            for (int i = 0; i < PPW; ++i)
                __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(src + i * X16_PIECE), (LDS_AS void*)(dst + i * X16_PIECE), 16,
                                                 0, 0);
        }
    }
    // spread schedule: chunk c is the next to be staged (the source wraps at NCHUNK); next<P>() issues its pieces at their slots
    __device__ __forceinline__ void stage(const int c) {
        stage_c = c;
        stage_src = src_c;
        src_c = src_c + 1 == NCHUNK ? 0 : src_c + 1;
    }
    template <int I>  // piece I of the PPW this wave stages of chunk stage_c
    __device__ __forceinline__ void issue_piece() {
        // The piece's scalar base and the lane offset are made opaque HERE: otherwise hipcc folds gsrc + voff into one per-lane
        // 64-bit pointer again (a v_lshl_add_u64 into a register pair per piece), or, with the zero-extension of voff hoisted
        // out of the block, no longer sees base + 32-bit offset and does the same.  (No immediate offset: see issue().)
        unsigned long long b = (unsigned long long)(gsrc + (size_t)stage_src * X16_CHUNK_BYTES + I * X16_PIECE);
        asm volatile("" : "+s"(b), "+v"(voff));
        const unsigned char* src = (const unsigned char*)(const GLOBAL_AS unsigned char*)b + voff;
        unsigned char* dst = ring + (stage_c % NBUF) * X16_CHUNK_BYTES + (wave * PPW + I) * X16_PIECE;
        __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)src, (LDS_AS void*)dst, 16, 0, 0);
    }
    __device__ __forceinline__ void prologue_issue(const int passes = 1) {
        limit = passes * NCHUNK;
        src_c = 0;
#pragma unroll
        for (int i = 0; i < NBUF - 1; ++i)
            if (i < limit) issue(i);
    }
    // a persistent workgroup is done: nothing of the stream may still be in flight towards its LDS when it exits
    __device__ __forceinline__ void drain() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }
    __device__ __forceinline__ void prologue_wait() {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
        chunk = 0;
        meets = 0;
        vm_cur = 0;
        vm_prev = 0;
        cur_addr = lds_addr0;
        nxt_addr = lds_addr0 + X16_CHUNK_BYTES;
        preload<0>();
    }
    template <int J>
    __device__ __forceinline__ void preload() {
        if constexpr (J < DEPTH - 1) {
            read_frag<J * X16_PIECE>(a[J], cur_addr);
            preload<J + 1>();
        }
    }
    // The wait of a rendezvous is COUNTED.  Chunk meets+1 was issued NBUF-2 rendezvous ago; vector-memory operations retire in
    // order (loads and stores share vmcnt on gfx9-family parts), so "at most K operations outstanding", K = what this wave has
    // issued SINCE THE LAST PIECE of that chunk, means its pieces have landed.  K = the (NBUF-3) newer chunks' loads plus the
    // stores the kernel reports through note_stores() AFTER that last piece.  A store reported before it (between the pieces of
    // a spread schedule, or ahead of them) is OLDER than the piece: counted, it would let vmcnt(K) pass with the piece still in
    // flight.  So the count restarts (restart_count) where a chunk's last piece is issued: behind the barrier for X16Issue<>, as
    // it always did, at the last slot for a spread schedule -- and at the rendezvous itself where it stages nothing (the tail;
    // stricter than needed), so that it restarts exactly once per period and vm_prev is the period before the current one.
    // The training kernels write 2-3 KiB per tile, and with a plain vmcnt(0) every rendezvous
    // also waited for the acknowledgement of the stores issued a tile ago (the write path runs near the HBM write bandwidth
    // there: the forward with SAVE took 1.58 ms against 0.92 ms without).  Safety: K must never exceed the true count, so only
    // stores that are issued UNCONDITIONALLY at their program point may be reported (dead waves write a dump record); loads and
    // stores the kernel does not report only make the wait stricter.  All of this folds at compile time (straight-line code).
    // THE COUNTED WAIT IS LOAD-BEARING IN EVERY BUILD.  The shipped rendezvous (X16_RV_RAW = 0) follows it with __syncthreads(),
    // and it is tempting to think that call's workgroup-scope release fence waits vmcnt(0) anyway (round 2's note said so, an
    // advisor repeated it, and early in round 3 the counted wait was compiled out of the shipped build on that belief).  It does
    // not: outside thread-group-split mode hipcc emits only the lgkmcnt part for that fence -- the shipped inference kernels show
    // `s_waitcnt lgkmcnt(..); s_barrier` with no vmcnt wait at 138 of 480 rendezvous (build/nerf_fwd_x16.s) -- so without the
    // wait below nothing orders a wave's LDS-DMA pieces of chunk meets+1 before the other waves read them.  The race almost
    // never shows (the chunk was issued two rendezvous earlier) and then shows as a parity failure once in a few hundred runs
    // (test_split_precision_mode_properties_at_full_size: 7.7e-4 instead of 5e-5).  tests/test_host_cpu.py now checks the
    // assembly: every rendezvous barrier of a stream kernel has a vmcnt wait in front of it.
    // -DX16_RV_RAW=1 (diagnostic) replaces __syncthreads() by a raw s_barrier between compiler barriers: what the barrier orders
    // needs no fence -- this wave's pieces of chunk meets+1 are awaited just above, and a wave's reads of chunk meets-1 (whose
    // buffer is overwritten next) were consumed by MFMAs a chunk ago.
    int vm_cur = 0, vm_prev = 0;  // reported stores since the count last restarted / in the period before that
    __device__ __forceinline__ void note_stores(const int n) { vm_cur += n; }
    __device__ __forceinline__ void restart_count() {
        vm_prev = vm_cur;
        vm_cur = 0;
    }
    template <int K>
    __device__ __forceinline__ static void wait_vm() {
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(K) : "memory");
    }
    __device__ __forceinline__ void rendezvous() {
        int newer = limit - 2 - meets;  // chunks issued after chunk meets+1: meets+2 .. min(limit-1, meets+NBUF-2)
        newer = newer < 0 ? 0 : (newer > NBUF - 3 ? NBUF - 3 : newer);
        int k = newer * PPW + vm_cur + (NBUF > 3 ? vm_prev : 0);
        if (k > 15) k = 15;
        static_for<0, 16>([&](auto k_c) {
            constexpr int K = decltype(k_c)::value;
            if (k == K) wait_vm<K>();  // this wave's pieces of chunk meets+1 have landed
        });
#if X16_RV_RAW
        __builtin_amdgcn_s_barrier();  // everyone's have; everyone has left chunk meets-1
        asm volatile("" ::: "memory");
#else
        __syncthreads();
#endif
        // the buffer of chunk meets-1 is free for chunk meets+NBUF-1
        if constexpr (SPREAD) {
            bool staged = false;
#ifndef X16_NODMA  // diagnostic build: the stream stops after the prologue (results are garbage, the timing is the point)
            if (meets + NBUF - 1 < limit) {
                stage(meets + NBUF - 1);  // next<P>() issues its pieces at their slots and restarts the count at the last
                staged = true;
            }
#endif
            if (!staged) restart_count();
        } else {
#ifndef X16_NODMA
            if (meets + NBUF - 1 < limit) issue(meets + NBUF - 1);
#endif
            restart_count();
        }
        ++meets;
    }
    // The fragment reads are issued from inline asm so that their completion can be awaited with a COUNTED
    // s_waitcnt lgkmcnt(DEPTH-1): hipcc's own bookkeeping waits lgkmcnt(0) here, i.e. for the prefetch it has just
    // issued, which puts a full LDS round trip in front of every other MFMA (45 % of the wave time parked).
    // LDS returns in order, so "at most DEPTH-1 younger operations outstanding" means this piece has landed; younger
    // compiler-issued LDS operations only make the wait more conservative.  The wait names the fragment as "+v", so
    // the consuming MFMA cannot be scheduled above it.
    template <int OFF>
    __device__ __forceinline__ void read_frag(frag& dst, const unsigned addr) {
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF) : "memory");
    }
    template <int YOUNGER = DEPTH - 1>  // fragment reads issued after this one that may still be in flight
    __device__ __forceinline__ void await_frag(frag& f) {
        asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(f) : "i"(YOUNGER));
    }
    // Fragment of stage-local piece P (stages are whole chunks, so P % X16_CH and P % DEPTH equal their
    // stream-global values).  LAST/NP: the final stage must not prefetch past the end of the stream.
    // EXTRA: LDS reads of the caller's own (inline asm, not awaited by it) that are YOUNGER than piece P's read and may still
    // be in flight here.  LDS returns in order, so they sit between piece P and the prefetches in the queue and the counted
    // wait has to allow for them, or it would wait for them and for the prefetch behind them as well.  Reads the caller issues
    // just before next<P0>() are younger than the pieces P0 .. P0 + DEPTH - 2 (read before them) and older than piece
    // P0 + DEPTH - 1, which next<P0>() itself reads: the caller passes EXTRA to exactly those DEPTH - 1 calls, and its reads
    // have landed once next<P0 + DEPTH - 1>() returns.
    static constexpr int depth = DEPTH;
    template <bool LAST, int NP, int P, int EXTRA = 0>
    __device__ __forceinline__ frag next() {
        if (P % X16_CH == RV) {
            X16_T(const unsigned long long r0 = x16_now();)
            rendezvous();
            X16_T(t_rv += x16_now() - r0;)
        }
        // the pieces of the staged chunk whose slot this is (stage_c < 0: none staged -- the stream's tail issues nothing)
        if constexpr (SPREAD)
            static_for<0, PPW>([&](auto i_c) {
                constexpr int I = decltype(i_c)::value;
                if constexpr (SCHED::at(I) == P % X16_CH)
                    if (stage_c >= 0) {
                        issue_piece<I>();
                        if constexpr (I == PPW - 1) {  // the chunk's last piece: the counted waits count from here
                            restart_count();
                            stage_c = -1;
                        }
                    }
            });
        constexpr int Q = P + DEPTH - 1;
#ifdef X16_NOLDS  // diagnostic build: no fragment reads at all (garbage results)
        if ((P + 1) % X16_CH == 0) ++chunk;
        return a[0];
#endif
        if (!(LAST && Q >= NP)) {
            const unsigned addr = (Q % X16_CH < P % X16_CH) ? nxt_addr : cur_addr;
            read_frag<(Q % X16_CH) * X16_PIECE>(a[Q % DEPTH], addr);
        }
        // at the stream's tail fewer reads are in flight behind this one: the count shrinks with them
        constexpr int younger = (LAST && NP - 1 - P < DEPTH - 1) ? NP - 1 - P : DEPTH - 1;
        static_assert(younger + EXTRA <= 15, "lgkmcnt is a 4-bit counter");
        await_frag<younger + EXTRA>(a[P % DEPTH]);
        const frag r = a[P % DEPTH];
        if ((P + 1) % X16_CH == 0) {
            ++chunk;
            cur_addr = nxt_addr;
            nxt_addr = lds_addr0 + ((chunk + 1) % NBUF) * X16_CHUNK_BYTES;
        }
        return r;
    }
    // A prefetch that nothing consumes must not be issued (LAST): its destination registers are dead to the compiler, which
    // hands them to other values while the read is still in flight -- the data then lands on top of them (seen in the
    // fused renderer block: store addresses overwritten by weight bytes, i.e. wild stores).  Where the code cannot know at
    // compile time whether the stream continues (a rolled loop over passes: the value is loop-carried, so its registers
    // stay reserved inside the loop), settle() after the loop retires the last prefetch before the registers are reused.
    // A RUN-TIME condition around read_frag / await_frag is not an option: the branch makes the fragment a phi and hipcc
    // copies the (not yet landed) registers ahead of the wait.
    __device__ __forceinline__ void settle() {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]));
#pragma unroll
        for (int i = 1; i < DEPTH; ++i) asm volatile("" : "+v"(a[i]));  // every slot stays reserved up to the wait
    }
};

// LeakyReLU(0.2) = max(a, 0.2 a) in two instructions.  As fmaxf() hipcc emits three: IEEE maxnum wants canonical inputs, and an
// accumulator read is not known to be one, so a v_max_f32 a, a, a goes in front (768 v_max for 384 activations in the C = 256
// renderer block).  A NaN propagates through v_max_f32 as through the three-instruction form, quieted.
__device__ __forceinline__ float x16_lrelu02(const float a) {
    const float b = 0.2f * a;
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// one float from LDS, issued from inline asm and NOT awaited: LDS returns in order, so the value has landed once a fragment read
// issued after it has been awaited (the caller then pins it with asm volatile("" : "+v"(dst)) before the first use)
template <int OFF>
__device__ __forceinline__ void x16_bias_read(float& dst, const unsigned addr) {
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF) : "memory");
}

// positional-encoding channel `ch` (0..63) via v_sin_f32 on a two-term phase in revolutions.  The three
// coordinates travel as separate scalars and are picked with selects: with float[3] arguments hipcc turned the
// runtime `dim` into an index into a private-memory copy (28 B/lane of scratch, 117 MB of traffic per launch).
__device__ __forceinline__ float pick3(const int d, const float a, const float b, const float c) {
    const float ab = d == 0 ? a : b;
    return d == 2 ? c : ab;
}
__device__ __forceinline__ float pe_fast(const float p0, const float p1, const float p2, const float h0, const float h1,
                                         const float h2, const float l0, const float l1, const float l2, const int ch) {
    const int cc = ch < 3 ? 0 : ch - 3;
    const int k = cc / 6, w = cc % 6, dim = w >= 3 ? w - 3 : w;
    const float sc = (float)(1 << k);
    const float hi = pick3(dim, h0, h1, h2), lo = pick3(dim, l0, l1, l2);
    // The phase is folded to [-1/4, 1/4] revolutions BEFORE the low part is added, every step of the fold exact in fp32
    // (hi * sc and lo * sc scale by a power of two; t is a fraction; 1/2 - |t| and 1/4 - |t| subtract numbers within a factor of
    // two of each other wherever the result is near zero): next to a zero crossing the argument of v_sin_f32 is then small and
    // keeps its low bits.  As fract(hi * sc) + lo * sc (+ 1/4) the sum was rounded at the scale of 1/2 or 1 -- 3e-8 revolutions,
    // 2e-7 in the sine, three bf16 ulps of a value of 1e-5 (tests/test_gpu_x16_stagewise.py: the PE tiles).
    const float u = __builtin_amdgcn_fractf(hi * sc);
    const float t = u - (u >= 0.5f ? 1.0f : 0.0f);                 // [-1/2, 1/2)
    const float at = __builtin_fabsf(t), ls = lo * sc;
    const float sl = t < 0.0f ? -ls : ls;                         // the low part, signed along |t|
    const bool far = at > 0.25f;
    const float ts = far ? 0.5f - at : at;                        // sin(2 pi t) = sign(t) sin(2 pi ts), ts in [0, 1/4]
    const float rs = (t < 0.0f ? -1.0f : 1.0f) * (ts + (far ? -sl : sl));
    const float rc = (0.25f - at) - sl;                           // cos(2 pi x) = sin(2 pi (1/4 - |x|))
    const float sv = __builtin_amdgcn_sinf(w >= 3 ? rc : rs);
    const float raw = pick3(ch, p0, p1, p2);
    return ch < 3 ? raw : (ch >= N3DT_PE_DIM ? 0.0f : sv);
}

// the sample position as a phase in revolutions, hi + lo, so that the 2^k scaling of the encoder stays exact
__device__ __forceinline__ void pe_phase(const float p, float& hi, float& lo) {
    const float inv2pi_hi = 0.15915494f, inv2pi_lo = 6.4206383e-09f;  // 1/(2 pi) = 0.159154936671257 (the float) + lo
    hi = p * inv2pi_hi;
    lo = fmaf(p, inv2pi_hi, -hi) + p * inv2pi_lo;
}

// One (octave, axis) of the encoding: s = pe_fast's channel 3 + 6k + dim, c = its channel 3 + 6k + 3 + dim, for sc = 2^k and the
// axis' phase hi + lo.  pe_fast's operations in pe_fast's order on either value (same floats, -ffp-contract=off); what the two
// channels share -- the reduced phase u, t, |t| and the signed low part -- is computed once, nothing is decoded from a channel
// index and neither argument is formed to be thrown away.
__device__ __forceinline__ void pe_pair(const float hi, const float lo, const float sc, float& s, float& c) {
    const float u = __builtin_amdgcn_fractf(hi * sc);
    const float t = u - (u >= 0.5f ? 1.0f : 0.0f);                 // [-1/2, 1/2)
    const float at = __builtin_fabsf(t), ls = lo * sc;
    const float sl = t < 0.0f ? -ls : ls;
    const bool far = at > 0.25f;
    const float ts = far ? 0.5f - at : at;
    const float rs = (t < 0.0f ? -1.0f : 1.0f) * (ts + (far ? -sl : sl));
    const float rc = (0.25f - at) - sl;
    s = __builtin_amdgcn_sinf(rs);
    c = __builtin_amdgcn_sinf(rc);
}

// Byte offset of channel ch (0..63) of sample 0 in a wave's four lane-linear PE pieces (piece ks = the B fragment of k-step ks,
// lane (c, h) element j = channel 16 ks + 8 (j >> 2) + 4 h + (j & 3)); sample c sits 16 c bytes further on.
constexpr int pe_slot_offset(const int ch) { return (ch / 16) * X16_PIECE + 512 * ((ch % 8) / 4) + 8 * ((ch % 16) / 8) + 2 * (ch % 4); }

// The whole encoding of a wave's 32 samples into its four B fragments.  Both lanes of a sample (c, h = 0 / 1) hold its position
// p.  Ownership is by OCTAVE half, not by fragment slot: lane (c, h) encodes octaves k = j + 5 h, j = 0 .. 4, on all three
// axes -- 15 pe_pair calls, 30 sines, every one of them used -- i.e. the consecutive channels 3 + 30 h .. 32 + 30 h, and the
// h = 0 lane adds the raw coordinates (channels 0 .. 2), the h = 1 lane the zero of channel 63.  The values reach their
// fragment slots through the wave's 4 KiB LDS copy (pe_lane = the copy + 16 lane; the skip stage reads it anyway): each is rounded as
// X16<PREC>::pack rounds it, channel pairs (even, odd) share a dword and go out as one 32-bit store, the seams (channels 2, 3
// and 32 on h = 0, 33 on h = 1) as 16-bit stores; the destination of a store is one of two compile-time offsets, picked by h.
// To keep the halves in lockstep without a branch the h = 1 lane repeats two of its stores (same value, same address).  Then
// four ds_read_b128 fetch the lane's fragments; LDS executes a wave's operations in order, so nothing waits in between.  The
// reads are NOT awaited here: the caller retires them with pe_settle() before the first use.
template <int PREC>
__device__ __forceinline__ void pe_encode(const float (&p)[3], const int h, unsigned char* pe_lane,
                                          typename X16<PREC>::frag (&pe)[4]) {
    float rh[3], rl[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pe_phase(p[i], rh[i], rl[i]);
    float e[30];  // e[6 j + w] = channel 3 + 30 h + 6 j + w
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const float sc = h ? (float)(32 << j) : (float)(1 << j);  // 2^(j + 5 h): hi * sc and lo * sc are pe_fast's products
#pragma unroll
        for (int dim = 0; dim < 3; ++dim) pe_pair(rh[dim], rl[dim], sc, e[6 * j + dim], e[6 * j + 3 + dim]);
    }
    LDS_AS unsigned char* const own = (LDS_AS unsigned char*)pe_lane;  // the lane's own 16 bytes of piece 0
    LDS_AS unsigned char* const row = own - 512 * h;                   // sample c's 16 bytes on the h = 0 side
    typedef unsigned __attribute__((may_alias)) u32;
    typedef unsigned short __attribute__((may_alias)) u16;
    // h = 0: channels 0, 1 = p0, p1;  h = 1: channels 62, 63 = e29, 0
    *(LDS_AS u32*)(row + (h ? pe_slot_offset(62) : pe_slot_offset(0))) = x16_cvt2<PREC>(h ? e[29] : p[0], h ? 0.0f : p[1]);
    // h = 0: channel 2 = p2;  h = 1: channel 33 = e0
    *(LDS_AS u16*)(row + (h ? pe_slot_offset(33) : pe_slot_offset(2))) = (unsigned short)x16_cvt2<PREC>(h ? e[0] : p[2], 0.0f);
    // h = 0: channels 3 and 32;  h = 1: 33 and 62 once more
    *(LDS_AS u16*)(row + (h ? pe_slot_offset(33) : pe_slot_offset(3))) = (unsigned short)x16_cvt2<PREC>(e[0], 0.0f);
    *(LDS_AS u16*)(row + (h ? pe_slot_offset(62) : pe_slot_offset(32))) = (unsigned short)x16_cvt2<PREC>(e[29], 0.0f);
#pragma unroll
    for (int i = 0; i < 14; ++i)  // channels 4 + 2 i, 5 + 2 i (h = 0) / 34 + 2 i, 35 + 2 i (h = 1)
        *(LDS_AS u32*)(row + (h ? pe_slot_offset(34 + 2 * i) : pe_slot_offset(4 + 2 * i))) = x16_cvt2<PREC>(e[2 * i + 1], e[2 * i + 2]);
    const unsigned at = (unsigned)(size_t)own;
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\t"
                 "ds_read_b128 %2, %4 offset:2048\n\tds_read_b128 %3, %4 offset:3072"
                 : "=&v"(pe[0]), "=&v"(pe[1]), "=&v"(pe[2]), "=&v"(pe[3])
                 : "v"(at)
                 : "memory");
}
// the one wait of the encoder, before the first use of its fragments (which stay reserved up to here)
template <class FRAG>
__device__ __forceinline__ void pe_settle(FRAG (&pe)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pe[0]), "+v"(pe[1]), "+v"(pe[2]), "+v"(pe[3]));
}

enum { MODE_HIDDEN = 0, MODE_LINEAR = 1, MODE_DENSITY = 2, MODE_COMPOSITE = 3 };


// sum over the 32 lanes of a half-wave of 32 per-lane values: lane c ends with value index rev5(c)
// Step 1 (partner lane c ^ 16) is a row swap between two registers: v_permlane16_swap_b32 trades the odd 16-lane rows of v[2i]
// against the even rows of v[2i + 1], after which v[2i] + v[2i + 1] is own + partner's v[2i] on the lanes with bit 4 clear and
// partner's + own v[2i + 1] on the others -- the sums the select / ds_bpermute form makes, operands commuted on the upper rows
// (fp32 addition commutes: same bits), without the two selects and the LDS permute per pair.  Inline asm, not
// __builtin_amdgcn_permlane16_swap: with both results feeding one add this hipcc emits `v_add v, a, a` (the second result is
// lost).  The s_nop 1 in front is the two wait states gfx950 wants between a VALU write of either operand and the swap's read
// (the compiler cannot see into the string); the one behind, in front of the add that reads both results, is caution only
// (no documented need; the form was measured with it).
__device__ __forceinline__ float butterfly32(float (&v)[32], const int c) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float a = v[2 * i], b = v[2 * i + 1];
        asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
        v[i] = a + b;
    }
#pragma unroll
    for (int step = 1; step < 5; ++step) {
        const int m = 16 >> step;
        const bool bit = (c & m) != 0;
        const int n = 32 >> step;
#pragma unroll
        for (int i = 0; i < n / 2; ++i) {
            float keep = bit ? v[2 * i + 1] : v[2 * i];
            float send = bit ? v[2 * i] : v[2 * i + 1];
            v[i] = keep + __shfl_xor(send, m, 64);
        }
    }
    return v[0];
}

// ---------------------------------------------------------------------------------------------
// Saved tiles of the training path: a [sample][channel] image that the weight-gradient kernel reads TRANSPOSED.
//
// A 32x32 tile in "lane = sample" form is two fragments f0, f1: lane (c, h) element j of f_s holds
// X[channel 16s + 8(j>>2) + 4h + (j&3)][sample c] (the B-operand form the fused kernels keep activations in).
// The weight gradients dW = dZ^T X sum over SAMPLES, so their MFMA operands need "lane = channel" fragments (8 samples of
// one channel per lane).  The first version transposed every tile on the matrix pipe before storing it (two selection MFMAs,
// 8 v_cvt_pk, the MFMA -> VALU latency: 8 % more MFMAs in the training forward and in the dX chain).  gfx950 transposes on
// the way OUT of LDS instead (ds_read_b64_tr_b16), so the producers now store their fragments as they are:
//     tile image (2 KiB) = [32 samples][32 channels] 16-bit, 64-byte rows;  lane (c, h) writes f_s at 64 c + 32 s + 16 h
// (row c = [ch 0-3, 8-11, 4-7, 12-15 | ch 16-19, 24-27, 20-23, 28-31]).  dw_x16_body moves the image to LDS as it is (two 1 KiB
// LDS-DMA pieces) and reads it with x16_tr_frag below.
// ---------------------------------------------------------------------------------------------
// dst: per-lane pointer = tile + 64 * (lane & 31) + 16 * (lane >> 5)   (x16_image_lane_offset)
__device__ __forceinline__ int x16_image_lane_offset(const int lane) { return 64 * (lane & 31) + 16 * (lane >> 5); }
template <int PREC>
__device__ __forceinline__ void x16_image_store(const typename X16<PREC>::frag f0, const typename X16<PREC>::frag f1, unsigned char* dst) {
    typedef typename X16<PREC>::frag frag;
#if X16_NT_STORE
    __builtin_nontemporal_store(f0, reinterpret_cast<frag*>(dst));
    __builtin_nontemporal_store(f1, reinterpret_cast<frag*>(dst + 32));
#else
    *reinterpret_cast<frag*>(dst) = f0;
    *reinterpret_cast<frag*>(dst + 32) = f1;
#endif
}
// Per-lane LDS byte offset of the transposed reads inside a tile image: lane (r, h) of the 32x32x16 operand takes channel r,
// samples 16 s' + 8 h + 0..7 as two 4-sample blocks.  In a group of 16 lanes, lane 4q + p supplies the address of sample row q,
// channels 4p .. 4p+3 of the group's 16 (the 8-byte unit (p & 1) * 2 + (p >> 1) of the row's 32 bytes).  A 32-lane half covers
// 4 rows x 64 bytes = all 64 banks once: conflict-free.  Checked against exact integer data on the GPU (tools/tr_probe.hip).
__device__ __forceinline__ unsigned x16_tr_lane_offset(const int lane) {
    const int r = lane & 31, h = lane >> 5, q = (r & 15) >> 2, p = r & 3;
    return 64u * (8 * h + q) + 32u * (r >> 4) + 8u * ((p & 1) * 2 + (p >> 1));
}
// The same for an image whose rows hold the 32 channels in NATURAL order (row-major maps of the 2-D renderer moved to LDS as
// they are, train_x16.inc: rowmajor): channels 4p .. 4p+3 are the p-th 8-byte unit.
__device__ __forceinline__ unsigned x16_tr_lane_offset_natural(const int lane) {
    const int r = lane & 31, h = lane >> 5, q = (r & 15) >> 2, p = r & 3;
    return 64u * (8 * h + q) + 32u * (r >> 4) + 8u * p;
}
// The reads are issued from inline asm (x16_tr_issue) and retired by ONE s_waitcnt (x16_tr_settle) that names every destination:
// through the builtin hipcc orders them behind the LDS-DMA stream in flight (s_waitcnt vmcnt(0) in front of the first read of
// every stage -- the stages still loading are then waited for as well, and the pipeline is one stage deep).
template <int OFF>
__device__ __forceinline__ void x16_tr_issue(x16_u32x2& d, const unsigned lds_addr) {
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(d) : "v"(lds_addr), "i"(OFF) : "memory");
}
// four 64-bit reads = the two k-steps of one 32 x 32 tile image at LDS byte address tile_lane (x16_tr_lane_offset included)
struct X16TrTile {
    x16_u32x2 q[4];  // k-step sp: q[2 sp] (samples +0..3), q[2 sp + 1] (samples +4..7)
    template <int TILE_OFF>
    __device__ __forceinline__ void issue(const unsigned tile_lane) {
        x16_tr_issue<TILE_OFF>(q[0], tile_lane);
        x16_tr_issue<TILE_OFF + 256>(q[1], tile_lane);
        x16_tr_issue<TILE_OFF + 1024>(q[2], tile_lane);
        x16_tr_issue<TILE_OFF + 1280>(q[3], tile_lane);
    }
    __device__ __forceinline__ void pin() {  // the destinations stay reserved up to the wait (x16_tr_settle)
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(q[i]));
    }
    __device__ __forceinline__ bf16x8 frag(const int sp) const {
        const x16_u32x4 v = {q[2 * sp][0], q[2 * sp][1], q[2 * sp + 1][0], q[2 * sp + 1][1]};
        return __builtin_bit_cast(bf16x8, v);
    }
};
__device__ __forceinline__ void x16_tr_settle() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
