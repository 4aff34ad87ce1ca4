// Fused volumetric-render kernel, 16-bit MFMA mode (bf16 or f16 inputs, fp32 accumulate):
// the roofline path.
//
// One wavefront carries one block of 32 consecutive samples of a ray through the whole MLP with
// v_mfma_f32_32x32x16_{bf16,f16}, eight wavefronts per workgroup (two per SIMD).  Activations are
// kept TRANSPOSED, H^T [channel][sample]: the sample sits on the MFMA column (lane & 31), the
// channels in the accumulator registers.  A 32x32 accumulator tile, ReLU'd and packed to 16 bit,
// is then directly the B operand of the next layer's MFMAs (its k order is a fixed permutation,
// matched by the weight packing, cdna guide section 3), so activations never leave the register
// file and LDS carries only weights.
//
// Weights: one flat stream of 1 KiB pieces (one MFMA A fragment each, lane-linear) in execution
// order.  All waves of the workgroup consume the same stream; it is staged L2 -> LDS by LDS-DMA
// (global_load_lds_dwordx4) in 24-piece chunks, double buffered, one workgroup barrier per chunk.
// Every fragment read is a conflict-free lane-linear ds_read_b128.
//
// Epilogue per 32-sample block: density -> alpha -> in-block transmittance scan over the 32
// lanes -> weights; the RGB_layer_1 activations are weighted and reduced over the samples with a
// 5-step butterfly, so the only HBM traffic per block is one 196-float partial.
#include "x16_core.h"
#include "n3dt_launch.h"


#ifndef X16_SAVE_DEPTH
#define X16_SAVE_DEPTH 3  // fragments in flight per wave in the training forward (X16_DEPTH for the others)
#endif
#ifndef X16_FWD_ISSUE
#define X16_FWD_ISSUE 0, 1, 2  // x16_core.h X16Issue: the slots of the three pieces a wave stages per chunk
#endif
// One stage: out[N x 32] = W'[N x K] . in[K x 32] + bias (+ activation), NT = N/32 out tiles.
// The KPE leading k-steps take their B operand from the wave's PE fragments: registers (pe_reg,
// stage L0) or the wave's LDS copy (pe_lds, skip stage L5); the rest come from hin.
// The bias is the C operand of a tile's first weight MFMA (X16TileInit below).
// SAVE (training forward): every finished output tile is also written to HBM for the backward -- hidden
// tiles as [sample][channel] images (x16_core.h: x16_image_store) at sv.tile0 + 2 KiB * tile, the RGB_layer_1 activations
// lane-linear (lane = sample fragments) at sv.tile0 + 1 KiB * k-step.
template <int PREC>
struct X16SaveStage {
    unsigned char* tile0;  // per-lane pointer (image offset, or lane * 16 for the lane-linear fragments, included)
    unsigned* gate0;       // per-lane pointer to this layer's 6 gate words (64 words apart)
};

// Biases come from LDS.  Every wave copies the next stage's fp32 bias table (<= 1.5 KiB) into its own
// LDS slot by LDS-DMA a stage ahead (X16BiasLds::stage_in; complete two rendezvous waits later at the latest -- the first may
// still leave as many operations outstanding as stores were reported before the copy was issued -- and read no earlier than the
// stage's last tile).  Nothing of it is on vmcnt inside the stream: vmcnt retires in order, so a wait for a bias LOAD would also
// wait for every saved-tile store of the training forward issued before it (0.2 ms of its 1.65 ms, diagnostic build).
//
// A tile's accumulator starts as the bias itself, exact in fp32, with no instruction of the matrix pipe spent on it (an
// earlier form broadcast a hi/lo-split 16-bit copy of it with one extra MFMA per tile: 95 of 2 375 per block).  Accumulator
// register r of lane half h is row (r & 3) + 8 (r >> 2) + 4 h of the tile, so the 16 values of a lane are four groups of four
// consecutive floats, at float 32 ot + 8 j + 4 h of the table, j = 0 .. 3: four ds_read_b128, each a broadcast within a lane
// half.  They are issued from inline asm a TILE AHEAD into the register set the running tile parity picks, and not
// awaited: LDS returns in order, so they have landed once a fragment read issued after them has been awaited, which
// WeightStream::next does DEPTH - 1 pieces later (its EXTRA argument keeps the counted waits in between exact).
// The FIRST tile of a stage is the exception.  Its reads are issued behind the k-loop of the last tile of the stage before,
// under that tile's pack / store epilogue, and the stage begins with the one full LDS wait it has (settle): a last tile
// holds the whole input and 11/12 of the output of its layer, and a second register set across its k-loop does not fit the
// 256 registers of two waves per SIMD (28 - 132 bytes of scratch in every instantiation when it was tried).
// The training forward (SAVE) keeps the earlier form, in which one float per lane (row c of the tile), fetched a tile ahead,
// is split hi/lo and broadcast by one extra MFMA (template argument BIAS of x16_stage): from LDS with x16_bias_read
// (X16_BIAS_LDS_MFMA) -- 84 bytes of scratch with the second register set next to its save pointers, 16 without.  Its density
// stage loads its bias from global memory (X16_BIAS_GLOBAL_MFMA), as it always did.
enum { X16_BIAS_GLOBAL_MFMA = 0, X16_BIAS_LDS_MFMA = 1, X16_BIAS_LDS_C = 2 };
#define X16_BIAS_SLOT 1536  // bytes: 384 floats
struct X16BiasLds {
    unsigned char* slots;  // this wave's two slots (generic pointer, wave-uniform)
    unsigned addr;         // LDS byte address of slot 0 + 16 * (lane >> 5)   (X16_BIAS_LDS_MFMA: + 4 * (lane & 31))
    // table -> slot (+ at, in floats) by LDS-DMA: n floats (a multiple of 64), 256 B per instruction, lane-linear
    __device__ __forceinline__ void stage_in(const float* table, const int n, const int slot, const int lane, const int at = 0) const {
#pragma unroll
        for (int i = 0; i < 6; ++i)
            if (64 * i < n)
                __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(table + 64 * i + lane),
                                                 (LDS_AS void*)(slots + slot * X16_BIAS_SLOT + 4 * at + 256 * i), 4, 0, 0);
    }
    // LDS address (lane half included) of the table staged into `slot` at float `at`
    __device__ __forceinline__ unsigned at(const int slot, const int at = 0) const { return addr + slot * X16_BIAS_SLOT + 4 * at; }
};
// the bias of one output tile as the lane's 16 accumulator values; two sets, tile n of the kernel's running count uses set n & 1
struct X16TileInit {
    f32x4 q[2][4];
    // OFF: byte offset of the tile in the table (128 per tile); table: X16BiasLds::at()
    template <int SET, int OFF>
    __device__ __forceinline__ void issue(const unsigned table) {
        asm volatile("ds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\t"
                     "ds_read_b128 %2, %4 offset:%7\n\tds_read_b128 %3, %4 offset:%8"
                     : "=&v"(q[SET][0]), "=&v"(q[SET][1]), "=&v"(q[SET][2]), "=&v"(q[SET][3])
                     : "v"(table), "i"(OFF), "i"(OFF + 32), "i"(OFF + 64), "i"(OFF + 96)
                     : "memory");
    }
    // the set stays reserved up to here (volatile asm statements keep their order: this one stays behind the stream's waits)
    template <int SET>
    __device__ __forceinline__ void landed() {
        asm volatile("" : "+v"(q[SET][0]), "+v"(q[SET][1]), "+v"(q[SET][2]), "+v"(q[SET][3]));
    }
    // first tile of a stage: one full wait (the two weight prefetches in flight are older and had to land first anyway)
    template <int SET>
    __device__ __forceinline__ void settle() {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(q[SET][0]), "+v"(q[SET][1]), "+v"(q[SET][2]), "+v"(q[SET][3]));
    }
    template <int SET>
    __device__ __forceinline__ f32x16 get() const {
        f32x16 v;
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = q[SET][r >> 2][r & 3];
        return v;
    }
};
constexpr int X16_TILE_INIT_READS = 4;

// PAR: parity of the stage's first tile in the kernel's running tile count.  The caller has issued that tile's bias reads;
// NEXT: a stage follows, and this one issues the reads of ITS first tile (table next_lds) behind its last k-loop.
// bias: the stage's table in global memory (read by X16_BIAS_GLOBAL_MFMA only); bias_lds: X16BiasLds::at() of its LDS copy
template <int PREC, int WAVES, int KS, int KPE, int NT, int MODE, bool SAVE, int BIAS, int PAR, bool NEXT, class WS>
__device__ __forceinline__ void x16_stage(WS& ws, X16TileInit& ti, const float* __restrict__ bias, const unsigned bias_lds, const unsigned next_lds,
                                          const typename X16<PREC>::frag (&pe_reg)[4], const unsigned char* pe_lds,
                                          const typename X16<PREC>::frag (&hin)[24], typename X16<PREC>::frag (&hout)[24],
                                          float& aux, float* const po, const bool live, const int lane,
                                          const X16SaveStage<PREC>* sv = nullptr, const short relu_lo = 0) {
    typedef typename X16<PREC>::frag frag;
    static_assert(KS >= WS::depth, "a tile's bias reads are covered by the wait of its own k-step DEPTH - 1");
    const int h = lane >> 5, c = lane & 31;
    float red[32];
    unsigned gate_word = 0;
    constexpr bool PACKS = (MODE == MODE_HIDDEN || MODE == MODE_LINEAR);
    f32x16 acc;
    constexpr bool CINIT = BIAS == X16_BIAS_LDS_C, LB = BIAS == X16_BIAS_LDS_MFMA;
    // the two MFMA forms
    [[maybe_unused]] const frag ones = X16<PREC>::ones_frag();
    [[maybe_unused]] float bias_cur = 0.0f, bias_nxt = 0.0f;
    if constexpr (LB) {
        x16_bias_read<0>(bias_cur, bias_lds);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bias_cur));  // once per stage; the tiles' values travel a tile ahead
    } else if constexpr (!CINIT) {
        bias_cur = bias[c];
    }
    auto finish_half = [&](const int t, const int half) {  // registers 8*half .. 8*half+7 of tile t -> k-step 2t+half
        float v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = acc[8 * half + r];
        frag f = X16<PREC>::pack(v);
        if (MODE == MODE_HIDDEN) f = X16<PREC>::relu(f, relu_lo);
        hout[2 * t + half] = f;
    };
    static_for<0, NT>([&](auto ot_c) {
        constexpr int ot = decltype(ot_c)::value;
        constexpr int cs = (PAR + ot) & 1, ns = cs ^ 1;    // this tile's register set of ti, the next tile's
        constexpr bool FETCH = CINIT && ot + 1 < NT;       // the next tile's bias is read under this tile's MFMAs
        X16_T(const unsigned long long s0 = x16_now();)
        if constexpr (CINIT) {
            if constexpr (ot == 0) ti.template settle<cs>();
            if constexpr (FETCH) ti.template issue<ns, (ot + 1) * 128>(bias_lds);
            acc = ti.template get<cs>();  // landed and pinned a tile ago: C of the first weight MFMA
        } else {
            // acc = bias, broadcast over the samples, by ONE extra MFMA (hi/lo split keeps ~16 mantissa bits):
            // lane r of the lower half holds bias[ot*32 + r], fetched one tile ahead
            const frag bf = X16<PREC>::bias_frag(bias_cur, h == 0);
            if constexpr (LB) {
                if constexpr (ot + 1 < NT) x16_bias_read<(ot + 1) * 128>(bias_nxt, bias_lds);
            } else {
                if (ot + 1 < NT) bias_cur = bias[(ot + 1) * 32 + c];
            }
            f32x16 zero;
#pragma unroll
            for (int r = 0; r < 16; ++r) zero[r] = 0.0f;
            acc = X16<PREC>::mfma(bf, ones, zero);
        }
        X16_T(const unsigned long long s1 = x16_now(); const unsigned long long rv0 = ws.t_rv;)
        static_for<0, KS>([&](auto ks_c) {
            constexpr int ks = decltype(ks_c)::value;
            // the four reads just issued are younger than the pieces of k-steps 0 .. DEPTH - 2, whose waits therefore allow
            // four more operations in flight; the wait of k-step DEPTH - 1 is the one that covers them
            const frag a_cur = ws.template next<MODE == MODE_COMPOSITE, NT * KS, ot * KS + ks,
                                                (FETCH && ks < WS::depth - 1) ? X16_TILE_INIT_READS : 0>();
            frag b;
            if (ks < KPE) {
                if (pe_lds) b = *reinterpret_cast<const frag*>(pe_lds + ks * X16_PIECE);
                else b = pe_reg[ks < 4 ? ks : 0];
            } else {
                b = hin[ks >= KPE ? ks - KPE : 0];
            }
            acc = X16<PREC>::mfma(a_cur, b, acc);
        });
        // landed: the reads are older than the fragment awaited at k-step DEPTH - 1 of the loop above
        if constexpr (FETCH) ti.template landed<ns>();
        else if constexpr (CINIT && NEXT && ot + 1 == NT) ti.template issue<ns, 0>(next_lds);  // awaited by the next stage's settle
        if constexpr (LB && ot + 1 < NT) {
            // landed likewise (the accumulator rides along: the statement then cannot move ahead of the loop's last MFMA)
            asm volatile("" : "+v"(bias_nxt), "+v"(acc));
            bias_cur = bias_nxt;
        }
        X16_T(const unsigned long long s2 = x16_now();)
        if (PACKS) {
            finish_half(ot, 0);
            finish_half(ot, 1);
        }
        if constexpr (SAVE && PACKS) {
            // (unconditional -- dead waves write a dump record -- and reported: the stream's rendezvous waits are counted)
#ifndef X16_DIAG_NOIMG
            x16_image_store<PREC>(hout[2 * ot], hout[2 * ot + 1], sv->tile0 + ot * 2 * X16_PIECE);
            ws.note_stores(2);
#endif
#ifndef X16_DIAG_NOGATE
            // ReLU gates of the backward chain: bit 8*half + j of this tile's half-word = "stored activation > 0" of accumulator
            // register 8*half + j (same lane, same tile, same register in nerf_bwd_x16_kernel); two tiles share a 32-bit word
            unsigned m = 0;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const s16x8 hv = __builtin_bit_cast(s16x8, hout[2 * ot + half]);
#pragma unroll
                for (int j = 0; j < 8; ++j) m |= (hv[j] != 0 ? 1u : 0u) << (8 * half + j);
            }
            // (v_pk_min_u16 + v_dot2_u32_u16 per packed pair would be 16 operations per tile instead of ~48, but hipcc expands
            // the packed min into compares and selects anyway and the dot2 result came out wrong on gfx950: not used)
            if constexpr (ot & 1) {
                __builtin_nontemporal_store(gate_word | (m << 16), sv->gate0 + (ot >> 1) * 64);
                ws.note_stores(1);
            } else {
                gate_word = m;
            }
#endif
        }
        if (MODE == MODE_DENSITY) {
            aux = acc[0];  // row 0 of the tile, valid on lanes with h == 0
        } else if (MODE == MODE_COMPOSITE) {
            // weighted RGB_layer_1 activations; two tiles (32 values) feed one butterfly over the samples
#pragma unroll
            for (int r = 0; r < 16; ++r) red[(ot & 1) * 16 + r] = fmaxf(acc[r], 0.0f) * aux;
            if constexpr (SAVE) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    float v[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) v[r] = fmaxf(acc[8 * half + r], 0.0f);
                    __builtin_nontemporal_store(X16<PREC>::pack(v), reinterpret_cast<frag*>(sv->tile0 + (2 * ot + half) * X16_PIECE));
                }
                ws.note_stores(2);
            }
            if (ot & 1) {
                float s = butterfly32(red, c);
                // bit-reversed lane index = which of the 32 reduced values this lane ended up with
                const int v = ((c & 1) << 4) | ((c & 2) << 2) | (c & 4) | ((c & 8) >> 2) | ((c & 16) >> 4);
                const int reg = v & 15, tile = (ot - 1) + (v >> 4);
                if (live) po[tile * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h] = s;
            }
        }
        X16_T(const unsigned long long s3 = x16_now(); ws.t_bias += s1 - s0; ws.t_mfma += (s2 - s1) - (ws.t_rv - rv0); ws.t_epi += s3 - s2;
              if (ws.tl && ws.tile_no >= 20 && ws.tile_no < 33 && (threadIdx.x & 63) == 0) {
                  ws.tl[4 + 2 * (ws.tile_no - 20)] = (float)(s1 & 0xFFFFFF);
                  ws.tl[5 + 2 * (ws.tile_no - 20)] = (float)(s2 & 0xFFFFFF);
              }
              ++ws.tile_no;)
    });
}

// What the training forward leaves in HBM per 32-sample block (bf16 fused training path, train_x16.hip):
//   xT   X16_XT_TILES tiles of 2 KiB: PE (2 tiles) | H0 .. H7 (12 tiles each), [sample][channel] images (x16_core.h)
//   gS   12 lane = sample fragments of relu(RGB_layer_1)
//   geo  density pre-activation [32] | plane distance [32]
//   gates  8 layers x 6 words x 64 lanes: the sign bits of H0 .. H7 in accumulator order (the dX chain's ReLU gates)
struct X16TrainSave {
    unsigned char* xT;
    unsigned char* gS;
    float* geo;
    unsigned* gates;
};

template <int PREC, int WAVES, bool SAVE = false>
__device__ __forceinline__ void nerf_fwd_x16_body(
    const N3dtGeom& g, const unsigned char* __restrict__ packed, const float* __restrict__ fold, const float* __restrict__ xy,
    const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ Kinv, const float* __restrict__ t_rand,
    float* __restrict__ part, float* __restrict__ wlocal, int bpr, long total_blocks, unsigned char* lds, const int wave,
    const X16TrainSave tsv = X16TrainSave{nullptr, nullptr, nullptr, nullptr}) {
    typedef typename X16<PREC>::frag frag;
    const int lane = threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;
    X16_T(const unsigned long long t_entry = x16_now();)  // the head: kernel entry .. behind prologue_wait()

    // (the training forward's prefetch depth is its own switch: depth 2 frees four registers and measured the same, 1.32 against 1.32 ms)
    // (the inference kernels issue the stream's LDS-DMA pieces between the MFMAs, X16_FWD_ISSUE; the training forward keeps them
    // behind the barrier: its A/B has not been run)
    typedef WeightStream<PREC, WAVES, X16_NCHUNK, X16_NBUF, SAVE ? X16_SAVE_DEPTH : X16_DEPTH,
                         std::conditional_t<SAVE, X16Issue<>, X16Issue<X16_FWD_ISSUE>>> WS;
    WS ws;
    if constexpr (SAVE) {
        ws.gsrc = packed + (size_t)wave * WS::PPW * X16_PIECE + lane * 16;
    } else {  // scalar base + lane offset (X16_FWD_ISSUE)
        ws.gsrc = packed + (size_t)wave * WS::PPW * X16_PIECE;
        ws.voff = lane * 16;
    }
    ws.ring = lds;
    ws.lds_addr0 = (unsigned)(size_t)(LDS_AS unsigned char*)lds + lane * 16;
    ws.wave = wave;
    ws.prologue_issue();  // the sampler / encoder below runs under these loads
    // per-wave LDS copy of the PE fragments for the skip stage: 4 lane-linear 1 KiB pieces
    unsigned char* pe_lds = lds + X16_NBUF * X16_CH * X16_PIECE + (size_t)wave * 4 * X16_PIECE + lane * 16;

    // block bookkeeping: the wave handles one 32-sample block
    long blk = (long)blockIdx.x * WAVES + wave;
    // (wave-uniform, and held as a scalar on purpose: as a lane mask it may be given VCC for the whole stream, and the training
    // forward's ReLU-gate compares then queue on one SGPR pair -- 550 s_nop per block when it happened)
    const bool live = __builtin_amdgcn_readfirstlane((int)(blk < total_blocks)) != 0;
    if (!live) blk = total_blocks - 1;
    float* const po = part + (size_t)blk * N3DT_PART_STRIDE;
    float dist, zval;
    frag pe[4];
    const int sb = (int)(blk % bpr);
    const long ray0 = blk / bpr;  // the wave's global ray
    const int ray = (int)(ray0 % g.n_rays);
    const int frame = (int)(ray0 / g.n_rays);
    {
        float p[3];
        n3dt_sample_point(g, xy, R, T, Kinv, t_rand, frame, ray, sb * X16_BS + c, p, dist, zval);
        // every (octave, axis) once, by octave half, through the wave's LDS copy into the fragments (x16_core.h); the reads
        // are in flight from here to pe_settle()
        pe_encode<PREC>(p, h, pe_lds, pe);
    }
    const float* fb = fold + (size_t)__builtin_amdgcn_readfirstlane(frame) * N3DT_FOLD_STRIDE;
    // include_vd: the merged RGB stage's bias is per RAY (frame entry + view-direction term; the table sits behind the fold table,
    // n3dt_layout.h)
    const float* b10 = fb + n3dt_bias_offset(10);
    if (g.vd_dim > 0) b10 = fold + n3dt_rayfold_offset(g.batch) + (size_t)__builtin_amdgcn_readfirstlane((int)ray0) * N3DT_RAYFOLD_STRIDE;
    X16SaveStage<PREC> svs;
    unsigned char* xT_blk = nullptr;  // this block's xT tiles (+ the lane's image offset)
    // record of this block in the saved buffers; a dead wave writes the dump record behind the last block (every wave must
    // issue the stores the stream's counted waits are told about, x16_core.h)
    const long rec = live ? blk : total_blocks;
    if constexpr (SAVE) {
        xT_blk = tsv.xT + (size_t)rec * X16_XT_TILES * 2 * X16_PIECE + x16_image_lane_offset(lane);
        pe_settle(pe);
        x16_image_store<PREC>(pe[0], pe[1], xT_blk);
        x16_image_store<PREC>(pe[2], pe[3], xT_blk + 2 * X16_PIECE);
    }
    // output tile 0 of hidden layer l inside the block's xT record
    auto sv_hidden = [&](const int l) -> const X16SaveStage<PREC>* {
        if constexpr (SAVE) {
            svs.tile0 = xT_blk + (size_t)(2 + 12 * l) * 2 * X16_PIECE;
            svs.gate0 = tsv.gates + ((size_t)rec * 8 + l) * 6 * 64 + lane;
            return &svs;
        } else {
            return nullptr;
        }
    };
    // how a tile's bias reaches its accumulator (X16TileInit above)
    constexpr int BIAS = SAVE ? X16_BIAS_LDS_MFMA : X16_BIAS_LDS_C;
    constexpr int BIAS_DEN = BIAS == X16_BIAS_LDS_C ? X16_BIAS_LDS_C : X16_BIAS_GLOBAL_MFMA;
    // per-wave bias slots in LDS, filled a stage ahead (X16BiasLds above).  Hidden stage k reads slot k & 1; the density tile
    // (64 floats staged, 32 used) and the merged RGB stage's table share slot 0, filled while stage 7 runs: the density
    // stage is a single chunk, too short to stage anything under it.
    X16BiasLds bl{nullptr, 0u};
    constexpr int DEN_AT = 192;  // float offset of the density tile in slot 0, behind the 192 RGB biases
    bl.slots = lds + X16_NBUF * X16_CH * X16_PIECE + (size_t)WAVES * 4 * X16_PIECE + (size_t)wave * 2 * X16_BIAS_SLOT;
    bl.addr = (unsigned)(size_t)(LDS_AS unsigned char*)bl.slots + (BIAS == X16_BIAS_LDS_C ? 16 * h : 4 * c);
    bl.stage_in(fb + n3dt_bias_offset(0), 384, 0, lane);
    // the bias slot of hidden stage k, after staging the table(s) of the stage that follows it
    auto bias_slot = [&](const int k) -> unsigned {
        if (k < 7) {
            bl.stage_in(fb + n3dt_bias_offset(k + 1), 384, (k + 1) & 1, lane);
        } else {
            bl.stage_in(b10, 192, 0, lane);
            if constexpr (BIAS_DEN == X16_BIAS_LDS_C) bl.stage_in(fb + n3dt_bias_offset(8), 64, 0, lane, DEN_AT);
        }
        return bl.at(k & 1);
    };
    if constexpr (!SAVE) pe_settle(pe);  // the encoder's one wait, as late as its fragments allow
    ws.prologue_wait();  // (vmcnt(0): table 0 is in its slot)
    X16_T(const unsigned long long t_head = x16_now() - t_entry;)
    X16_T(if (wlocal && live) ws.tl = wlocal + (size_t)blk * X16_BS;)
    X16TileInit ti;
    if constexpr (BIAS == X16_BIAS_LDS_C) ti.template issue<0, 0>(bl.at(0));

    frag ha[24], hb[24];
    float aux;
    // FeaExt_module_0 (reference: NetWorks/models.py:69-71)
    x16_stage<PREC, WAVES, 4, 4, 12, MODE_HIDDEN, SAVE, BIAS, 0, true>(ws, ti, fb + n3dt_bias_offset(0), bias_slot(0), bl.at(1), pe, nullptr, ha, ha, aux, po, live, lane, sv_hidden(0));
    // FeaExt_module_1..7 with the skip concat after layer 4 (models.py:72-76).  Fully unrolled on purpose: rolling the
    // identical 384->384 layers into a loop (tried: one-layer body + register copy, two-layer ping-pong body) makes the
    // register allocator spill 120-270 VGPRs across the back edge and runs 1.7x slower.
    x16_stage<PREC, WAVES, 24, 0, 12, MODE_HIDDEN, SAVE, BIAS, 0, true>(ws, ti, fb + n3dt_bias_offset(1), bias_slot(1), bl.at(0), pe, nullptr, ha, hb, aux, po, live, lane, sv_hidden(1));
    x16_stage<PREC, WAVES, 24, 0, 12, MODE_HIDDEN, SAVE, BIAS, 0, true>(ws, ti, fb + n3dt_bias_offset(2), bias_slot(2), bl.at(1), pe, nullptr, hb, ha, aux, po, live, lane, sv_hidden(2));
    x16_stage<PREC, WAVES, 24, 0, 12, MODE_HIDDEN, SAVE, BIAS, 0, true>(ws, ti, fb + n3dt_bias_offset(3), bias_slot(3), bl.at(0), pe, nullptr, ha, hb, aux, po, live, lane, sv_hidden(3));
    x16_stage<PREC, WAVES, 24, 0, 12, MODE_HIDDEN, SAVE, BIAS, 0, true>(ws, ti, fb + n3dt_bias_offset(4), bias_slot(4), bl.at(1), pe, nullptr, hb, ha, aux, po, live, lane, sv_hidden(4));
    x16_stage<PREC, WAVES, 28, 4, 12, MODE_HIDDEN, SAVE, BIAS, 0, true>(ws, ti, fb + n3dt_bias_offset(5), bias_slot(5), bl.at(0), pe, pe_lds, ha, hb, aux, po, live, lane, sv_hidden(5));
    x16_stage<PREC, WAVES, 24, 0, 12, MODE_HIDDEN, SAVE, BIAS, 0, true>(ws, ti, fb + n3dt_bias_offset(6), bias_slot(6), bl.at(1), pe, nullptr, hb, ha, aux, po, live, lane, sv_hidden(6));
    x16_stage<PREC, WAVES, 24, 0, 12, MODE_HIDDEN, SAVE, BIAS, 0, true>(ws, ti, fb + n3dt_bias_offset(7), bias_slot(7), bl.at(0, DEN_AT), pe, nullptr, ha, hb, aux, po, live, lane, sv_hidden(7));
    // density head on h7 (models.py:78,84); the bias rides in the accumulator.  Its one tile is tile 96 of the running count
    // and fetches the first RGB tile's bias, which therefore starts on parity 1.
    x16_stage<PREC, WAVES, 24, 0, 1, MODE_DENSITY, false, BIAS_DEN, 0, true>(ws, ti, fb + n3dt_bias_offset(8), bl.at(0, DEN_AT), bl.at(0), pe, nullptr, hb, ha, aux, po, live, lane);
    // alpha, in-block transmittance and weights (reference: NetWorks/utils.py:273-289)
    {
        float sp = __shfl(aux, c, 64);  // row 0 lives on the h == 0 half
        if constexpr (SAVE) {
            if (live && h == 0) {
                tsv.geo[(size_t)blk * 64 + c] = sp;
                tsv.geo[(size_t)blk * 64 + 32 + c] = dist;
            }
        }
        float sigma = fmaxf(sp, 0.0f);
        float alpha = 1.0f - expf(-sigma * dist);
        float x = 1.0f - alpha + 1e-10f;
        float Tl = n3dt_exclusive_prod<32>(x, c);
        float w = alpha * Tl;
        float s0 = w, s1 = w * zval;
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) {
            s0 += __shfl_xor(s0, off, 32);
            s1 += __shfl_xor(s1, off, 32);
        }
        float tprod = __shfl(Tl * x, 31, 32);
        if (live && lane == 0) {
            po[N3DT_G + 0] = s0;
            po[N3DT_G + 1] = s1;
            po[N3DT_G + 2] = tprod;
            po[N3DT_G + 3] = 0.0f;
        }
#ifndef X16_STAMP
        if (live && wlocal && h == 0) wlocal[(size_t)blk * X16_BS + c] = w;
#endif
        aux = w;
    }
    // RGB_layer_0 -> RGB_layer_1 as ONE merged 192 x 384 layer on h7 (no activation sits between them, models.py:79-81;
    // merged matrix and bias built by pack / fold), relu, weighted by the sample weights and reduced over the samples
    if constexpr (SAVE) {
        svs.tile0 = tsv.gS + (size_t)rec * 12 * X16_PIECE + lane * 16;
        svs.gate0 = nullptr;
    }
    x16_stage<PREC, WAVES, 24, 0, 6, MODE_COMPOSITE, SAVE, BIAS, 1, false>(ws, ti, b10, bl.at(0), 0u, pe, nullptr, hb, ha, aux, po, live, lane,
                                                                               SAVE ? &svs : nullptr);
#ifdef X16_STAMP
    if (wlocal && lane == 0 && live) {
        float* dbg = wlocal + (size_t)blk * X16_BS;
        dbg[0] = (float)ws.t_bias;
        dbg[1] = (float)ws.t_mfma;
        dbg[2] = (float)ws.t_epi;
        dbg[3] = (float)ws.t_rv;
        dbg[30] = (float)t_head;  // (the tile timeline ends at slot 29: tiles 20 .. 32)
    }
#endif
}

template <int PREC, int WAVES>
__global__ __launch_bounds__(WAVES * 64, 1) void nerf_fwd_x16_kernel(
    N3dtGeom g, const unsigned char* __restrict__ packed, const float* __restrict__ fold, const float* __restrict__ xy,
    const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ Kinv, const float* __restrict__ t_rand,
    float* __restrict__ part, float* __restrict__ wlocal, int bpr, long total_blocks) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    nerf_fwd_x16_body<PREC, WAVES>(g, packed, fold, xy, R, T, Kinv, t_rand, part, wlocal, bpr, total_blocks, lds, wave);
}

// Training forward (bf16): the same body, leaving the activations behind (X16TrainSave)
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64, 1) void nerf_fwd_x16_train_kernel(
    N3dtGeom g, const unsigned char* __restrict__ packed, const float* __restrict__ fold, const float* __restrict__ xy,
    const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ Kinv, const float* __restrict__ t_rand,
    float* __restrict__ part, float* __restrict__ wlocal, int bpr, long total_blocks, X16TrainSave tsv) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    nerf_fwd_x16_body<N3DT_BF16, WAVES, true>(g, packed, fold, xy, R, T, Kinv, t_rand, part, wlocal, bpr, total_blocks, lds, wave,
                                                        tsv);
}

#ifndef X16_TRAIN_WAVES
#define X16_TRAIN_WAVES 8
#endif
extern "C" void n3dt_launch_nerf_fwd_x16_train(const N3dtGeom* g, const void* packed, const float* fold, const float* xy, const float* R,
                                               const float* T, const float* Kinv, const float* t_rand, float* part, float* wlocal,
                                               void* xT, void* gS, float* geo, void* gates, hipStream_t stream) {
    constexpr int WAVES = X16_TRAIN_WAVES;
    const int bpr = (g->n_samples + X16_BS - 1) / X16_BS;
    const long total = (long)g->batch * g->n_rays * bpr;
    const int grid = (int)((total + WAVES - 1) / WAVES);
    const size_t lds_bytes = X16_NBUF * X16_CH * X16_PIECE + (size_t)WAVES * 4 * X16_PIECE + (size_t)WAVES * 2 * X16_BIAS_SLOT;
    auto kern = nerf_fwd_x16_train_kernel<WAVES>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    X16TrainSave tsv{reinterpret_cast<unsigned char*>(xT), reinterpret_cast<unsigned char*>(gS), geo, reinterpret_cast<unsigned*>(gates)};
    hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVES * 64), lds_bytes, stream, *g, reinterpret_cast<const unsigned char*>(packed), fold, xy,
                       R, T, Kinv, t_rand, part, wlocal, bpr, total, tsv);
}

template <int PREC>
static void launch_x16(const N3dtGeom* g, const void* packed, const float* fold, const float* xy, const float* R, const float* T,
                       const float* Kinv, const float* t_rand, float* part, float* wlocal, hipStream_t stream) {
    constexpr int WAVES = 8;  // two waves per SIMD, <= 256 registers each
    const int bpr = (g->n_samples + X16_BS - 1) / X16_BS;
    const long total = (long)g->batch * g->n_rays * bpr;
    const int grid = (int)((total + WAVES - 1) / WAVES);
    // weight ring + the waves' PE copies + their two bias slots: 72 + 32 + 24 KiB, one workgroup per CU
    const size_t lds_bytes = X16_NBUF * X16_CH * X16_PIECE + (size_t)WAVES * 4 * X16_PIECE + (size_t)WAVES * 2 * X16_BIAS_SLOT;
    auto kern = nerf_fwd_x16_kernel<PREC, WAVES>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVES * 64), lds_bytes, stream, *g, reinterpret_cast<const unsigned char*>(packed),
                       fold, xy, R, T, Kinv, t_rand, part, wlocal, bpr, total);
}

extern "C" void n3dt_launch_nerf_fwd_x16(const N3dtGeom* g, int precision, const void* packed, const float* fold, const float* xy,
                                         const float* R, const float* T, const float* Kinv, const float* t_rand, float* part,
                                         float* wlocal, hipStream_t stream) {
    if (precision == N3DT_BF16) launch_x16<N3DT_BF16>(g, packed, fold, xy, R, T, Kinv, t_rand, part, wlocal, stream);
    else launch_x16<N3DT_F16>(g, packed, fold, xy, R, T, Kinv, t_rand, part, wlocal, stream);
}
