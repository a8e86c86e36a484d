// 3x3 / stride-1 / pad-1 convolution for channel counts that are multiples of 96 (the 96 / 192 / 384-channel branches of
// HRNet-W48): 96 output channels per block, 32-channel input slices.  Included by conv3x3_lds.hip (same kernel, so the
// convolutions of all branches of a stage module still go out as ONE grouped launch).
//
// Why a second form (round-1 counters, DESIGN.md §5): the 48-cout form re-stages the input slab once per 48 output channels
// and the weights once per 384-512 pixels -- 5.6 KB of LDS-DMA per MFLOP on the 96-channel branch, 15 one-KiB DMA
// instructions per wave and slice, 7 ds_read_b128 per 12 MFMAs, one block-wide barrier per 84 MFMAs that every wave leaves
// with an empty pipeline, and 3.6 % of the K loop spent on padding.  Here:
//   * block tile = 128*MR pixels x 96 couts (wave = 16*MR pixels x 96 couts: 6+MR ds_read_b128 per 6*MR MFMAs), input slices
//     of KS = 32 channels: K per slice = 9 x 32, one 32-wide MFMA chunk per tap, NO K padding; 3.3 KB of LDS-DMA per MFLOP.
//   * a stage = one kernel ROW of one slice (3 chunks, 18*MR MFMAs per wave).  LDS = 4 weight stage buffers (4 x 18 KiB) +
//     2 slab buffers (64-byte rows, 16-byte slots XOR-swizzled as in the KS = 32 form) + the 96 biases.
//   * weights run THREE stages ahead of their use and the next slice's slab one whole stage ahead of its first use, every
//     wave waits for its own pieces with a COUNTED vmcnt (allowing what it issued during the stage just finished) before the
//     stage barrier.  So whatever a wave reads in stage q+1 was already complete at barrier q: the first fragments of stage
//     q+1 are requested BEFORE barrier q+1 (weights always, pixels when the slab does not change), and a wave leaves the
//     barrier straight into MFMAs instead of into a burst of 8 x 7 LDS reads.
//   * fragment registers: the six weight fragments are a ring -- fragment j of chunk c+1 is requested right after the MFMAs
//     that consumed fragment j of chunk c were issued -- and the pixel fragments alternate between two sets: 24 + 8*MR
//     registers instead of two full sets (16*(6+MR)/2...), which is what lets 96 accumulators + the residual tile fit.
//   * the accumulators start at the bias (read from LDS: 24 registers less across the tile loop).
// K order: slice-major, tap, channel -- not the order of the 48-cout form or the generic kernel, so a convolution takes this
// form at EVERY batch size (128-pixel tiles, MR = 1, when a launch could not fill the chip) and results do not depend on
// the batch a crop arrives in.

// Output channels of a lane.  The packed weight row i = 4 g + r of fragment j holds output channel
//   N96_CH64 = 0:  g * 24 + j * 4 + r                         (24 contiguous channels: three 16-byte pieces 48 bytes apart per g)
//   N96_CH64 = 1:  (j >> 1) * 32 + g * 8 + (j & 1) * 4 + r    (8 contiguous channels in each 32-channel group: the four lanes
//                  of a pixel cover 64 contiguous bytes per load / store instruction instead of four scattered 16-byte pieces)
// pixel-fragment reads of the next chunk issued per MFMA group (1: the last one has two groups to land, 2: four)
#ifndef N96_XPG
#define N96_XPG 2
#endif
// fewer instructions in the chunk loop: one counted wait for all of a chunk's weight fragments instead of one per group, the
// three pixel-fragment addresses of a stage formed once, M0 not saved around the LDS-DMA
#ifndef N96_TRIM
#define N96_TRIM 1
#endif
#ifndef N96_CH64
#define N96_CH64 1
#endif
constexpr int N96_WST = 3 * 6 * 1024;                       // one weight stage: 3 taps x 6 fragments x 1 KiB
constexpr int N96_NWB = 4;                                  // weight stage buffers
constexpr int N96_SLAB = 44800;                             // one slab buffer: 700 rows of 64 B
constexpr int N96_SB = N96_NWB * N96_WST;                   // slab buffers start here
constexpr int N96_BIAS = N96_SB + 2 * N96_SLAB;             // 96 fp32 biases
constexpr int N96_LDS = N96_BIAS + 384;
static_assert(N96_LDS <= 160 * 1024, "LDS budget");
constexpr int N96_MAXROWS = N96_SLAB / 64;

template <int N>
__device__ __forceinline__ void n96_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}
// wait until at most n vector-memory operations of this wave are outstanding (n wave-uniform, 0..23; more: 23, stricter).
// s_waitcnt only takes an immediate, and a switch over it compiles into ~40 scalar instructions of flag juggling per stage
// entry: a computed jump into a table of (s_waitcnt vmcnt(k); s_branch end) pairs instead -- six scalar instructions.
__device__ __forceinline__ void n96_vmcnt_dyn(int n) {
    n = n < 23 ? n : 23;
    unsigned tmp;
    asm volatile("s_getpc_b64 s[100:101]\n\t"      // address of the next instruction (A)
                 "s_lshl_b32 %0, %1, 3\n\t"         // A + 0   8 bytes per table entry
                 "s_add_u32 %0, %0, 20\n\t"         // A + 4   the table starts at A + 20
                 "s_add_u32 s100, s100, %0\n\t"     // A + 8
                 "s_addc_u32 s101, s101, 0\n\t"     // A + 12
                 "s_setpc_b64 s[100:101]\n\t"       // A + 16
                 "s_waitcnt vmcnt(0)\n\ts_branch 46\n\t"
                 "s_waitcnt vmcnt(1)\n\ts_branch 44\n\t"
                 "s_waitcnt vmcnt(2)\n\ts_branch 42\n\t"
                 "s_waitcnt vmcnt(3)\n\ts_branch 40\n\t"
                 "s_waitcnt vmcnt(4)\n\ts_branch 38\n\t"
                 "s_waitcnt vmcnt(5)\n\ts_branch 36\n\t"
                 "s_waitcnt vmcnt(6)\n\ts_branch 34\n\t"
                 "s_waitcnt vmcnt(7)\n\ts_branch 32\n\t"
                 "s_waitcnt vmcnt(8)\n\ts_branch 30\n\t"
                 "s_waitcnt vmcnt(9)\n\ts_branch 28\n\t"
                 "s_waitcnt vmcnt(10)\n\ts_branch 26\n\t"
                 "s_waitcnt vmcnt(11)\n\ts_branch 24\n\t"
                 "s_waitcnt vmcnt(12)\n\ts_branch 22\n\t"
                 "s_waitcnt vmcnt(13)\n\ts_branch 20\n\t"
                 "s_waitcnt vmcnt(14)\n\ts_branch 18\n\t"
                 "s_waitcnt vmcnt(15)\n\ts_branch 16\n\t"
                 "s_waitcnt vmcnt(16)\n\ts_branch 14\n\t"
                 "s_waitcnt vmcnt(17)\n\ts_branch 12\n\t"
                 "s_waitcnt vmcnt(18)\n\ts_branch 10\n\t"
                 "s_waitcnt vmcnt(19)\n\ts_branch 8\n\t"
                 "s_waitcnt vmcnt(20)\n\ts_branch 6\n\t"
                 "s_waitcnt vmcnt(21)\n\ts_branch 4\n\t"
                 "s_waitcnt vmcnt(22)\n\ts_branch 2\n\t"
                 "s_waitcnt vmcnt(23)\n\ts_branch 0\n\t"
                 : "=&s"(tmp)
                 : "s"(n)
                 : "s100", "s101", "scc", "memory");
}

// LDS-DMA of 64 lanes x 16 B: source = wave-uniform base (SGPR pair) + per-lane 32-bit byte offset, destination = LDS byte
// address lds_dst (wave-uniform) + lane * 16.  Written out because the builtin, given base + offset, moves the base into a
// VGPR pair and adds there (two VALU ops and two registers per piece, and hipcc then keeps those pairs live across the loops).
// M0 is the compiler's: saved and restored around the statement (cdna_hip_programming.md 5.7).
__device__ __forceinline__ void n96_glds(const GLOBAL_AS char *base, unsigned voff, unsigned lds_dst) {
#ifdef N96_NODMA   // timing-only ablation (tools/c3n_test.hip): results are garbage
    return;
#endif
#if N96_TRIM
    // (M0 is not saved but declared clobbered: the compiler re-establishes it before its own uses -- its LDS-DMA builtins in the
    // prologue set it right before each use anyway; tests/test_build_invariants.py checks on the disassembly that nothing but
    // LDS-DMA reads M0 in this kernel)
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %2" ::"v"(voff), "s"(lds_dst), "s"(base) : "memory", "m0");
#else
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(lds_dst), "s"(base)
                 : "memory");
#endif
}

// CP (round 4): COMPACT enumeration of the M dimension -- tile t = real pixels [t BM, (t + 1) BM) of the tensor in (image, row, column)
// order, the pad column and pad row of the flat layout never enter a tile (on the 24x18 and 12x9 grids they are 9 % and 17 % of the
// flat pixels = of the MFMAs).  Input layout, slab, taps and the arithmetic per output pixel are unchanged (bit-identical results):
// a tile's slab is still one run of flat rows, from the first pixel's window start to the last one's end -- `slab_rows` rows,
// the longest such run of the geometry --, and a fragment's 16 lanes are 16 consecutive REAL pixels, so every pixel fragment has its
// own slab address and swizzle bits (measured on the flat enumeration: ~4 % of the loop, profiles/EXPERIMENTS.md) and the outputs their own rows.
template <int MR, bool CP, int DT>
__device__ __forceinline__ void c3n_run(const Conv3Problem &p_, const int nt, const int mt0, const int tiles_this_block,
                                        const int nb, char *smem) {
    constexpr bool PF = CP;   // one slab address per pixel fragment
    constexpr int NRB = 6, ROWB = 64, NT = 512, BM = 128 * MR, WST = N96_WST, SLABB = N96_SLAB;
    constexpr int NSP = (SLABB / 16 + NT - 1) / NT;   // slab LDS-DMA pieces per wave at most (6)
    constexpr int NSH = NSP / 2;                      // ... issued in part 0; the rest in part 1
    constexpr int NST = 3 * MR;                       // stores (and residual loads) per wave and tile
    static_assert(NSP == 6 && MR <= 4, "DMA slot plan");
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    // (scalar copies: the statements below clobber "memory", a field read through the reference would be re-loaded after each)
    const Conv3Problem p = p_;
    C3_T(t_entry0);   // (timing builds: the block's prologue = from here to the first stage)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
#ifndef N96_NOPRIO
    if (wave >= 4) __builtin_amdgcn_s_setprio(1);   // the younger wave of each SIMD (see conv3_run)
#endif
    const int m = CP ? nb * p.hw : nb * p.hpwp;   // pixels to produce: real ones / flat rows
    const int mtiles = (m + BM - 1) / BM;
    int ntile = mtiles - mt0;
    if (ntile > tiles_this_block) ntile = tiles_this_block;
    if (ntile <= 0) return;
    const int S = p.slices;
    const int slab_units = CP ? (MR == 1 ? p.slab_rows_small : p.slab_rows) * 4 : (BM + 2 * p.wp + 2) * 4;
    // compact index -> flat row (wave-uniform or per lane)
    auto flat_of = [&](int c) -> int {
        const int n_ = (int)(((unsigned long long)(unsigned)c * p.magic_hw) >> p.shift_hw);
        const int r_ = c - n_ * p.hw;
        const int ho_ = (int)(((unsigned long long)(unsigned)r_ * p.magic_w) >> p.shift_w);
        return n_ * p.hpwp + ho_ * p.wp + (r_ - ho_ * p.wd);
    };
    // flat row of M tile t's first pixel
    auto tile_first = [&](int t) -> int { return CP ? flat_of(t * BM) : t * BM; };
    const gcu16 in = (gcu16)p.in;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;

    // (SW = an opaque copy of swz made where the address is needed: hipcc would otherwise keep all nine offsets in registers)
#define N96_XOFF(C, SW) ((unsigned)((((C) / 3) * p.wp + ((C) % 3)) * ROWB) + ((((SW) >> (C)) & 1u) ? swz_step : 0))
    // per-lane byte offset of a slab piece's source relative to the slab's first row.  Unit u = k * 512 + tid is 16-byte
    // slot u % 4 of row u / 4, and bit 2 of that row does not depend on k, so piece k is piece 0 moved by 128 k rows (a
    // scalar add to the base); only the LAST piece has lanes beyond the slab, which re-read its last unit.
    const int kmax = (slab_units - 1) / NT;
    unsigned srel0, srel_tail;
    {
        const int r = tid >> 2;
        const int q = (tid & 3) ^ (((r >> 2) & 1) << 1);   // LDS slot u % 4 of row r holds source slot q
#ifdef N96_FAKE_BLOCKED   // TIMING-ONLY experiment (garbage results): every access shaped as if activations were stored [C/32][rows][32]
        srel0 = (unsigned)(r * 32 + q * 8) * 2u;
#else
        srel0 = (unsigned)(r * p.cin + q * 8) * 2u;
#endif
        int u = kmax * NT + tid;
        if (u >= slab_units) u = slab_units - 1;           // the buffer has room for the tail lanes
        const int r2 = u >> 2;
        const int q2 = (u & 3) ^ (((r2 >> 2) & 1) << 1);
#ifdef N96_FAKE_BLOCKED
        srel_tail = (unsigned)((r2 - kmax * 128) * 32 + q2 * 8) * 2u;
#else
        srel_tail = (unsigned)((r2 - kmax * 128) * p.cin + q2 * 8) * 2u;
#endif
    }
#ifdef N96_FAKE_BLOCKED
    const unsigned piece_rows_bytes = 128u * 32 * 2u;
    const size_t fb_ss = (size_t)nb * p.hpwp * 32;   // elements between 32-channel groups of one tensor
#else
    const unsigned piece_rows_bytes = 128u * p.cin * 2u;   // source distance of consecutive pieces
#endif
    const int nw_wave = (18 - wave + 7) >> 3;                     // weight pieces of this wave per stage: idx = wave + 8 t < 18
    int ns_wave = (slab_units - wave * 64 + NT - 1) / NT;         // slab pieces of this wave: k * 512 + wave * 64 < slab_units
    ns_wave = ns_wave < 0 ? 0 : (ns_wave > NSP ? NSP : ns_wave);
    const int ns_p0 = ns_wave < NSH ? ns_wave : NSH, ns_p1 = ns_wave - ns_p0;

    const int ch0 = N96_CH64 ? nt * 96 + g * 8 : nt * 96 + g * 24;
    constexpr int VSTEP = N96_CH64 ? 64 : 16;   // byte distance of the lane's three 16-byte pieces
    const gu16 out = (gu16)p.out;
    const bool has_res = p.res != nullptr;
    const gcu16 res = has_res ? (gcu16)p.res : in - (size_t)(p.wp + 1) * p.cin;   // (no residual: the zero guard rows)
    const GLOBAL_AS char *const wsrc_nt = (const GLOBAL_AS char *)p.w + (size_t)nt * S * (3 * WST);
    const unsigned bias_a = lds0 + N96_BIAS + (N96_CH64 ? g * 32 : g * 96);
    const unsigned lane16 = lane * 16;

#ifdef HRN_C3_TIMING
    int t_pro_issue = 0;
#endif
    // ---- prologue: weight stages 0..2 (slice 0), the slab of (tile 0, slice 0), the biases
    {
#pragma unroll
        for (int st = 0; st < 3; ++st)
#pragma unroll
            for (int t = 0; t < 3; ++t)
                if (t < nw_wave) {
                    const int idx = wave + 8 * t;
                    glds16(wsrc_nt + (size_t)st * WST + idx * 1024 + lane * 16, smem + st * WST + idx * 1024);
                }
        const long row0 = (long)tile_first(mt0) - p.wp - 1;   // guard rows make negative / overrun rows valid
#ifdef N96_FAKE_BLOCKED
        const GLOBAL_AS char *ssrc = (const GLOBAL_AS char *)(in + (row0 < 0 ? 0 : row0) * 32);
#else
        const GLOBAL_AS char *ssrc = (const GLOBAL_AS char *)(in + row0 * p.cin);
#endif
#pragma unroll
        for (int k = 0; k < NSP; ++k)
            if (k < ns_wave) glds16(ssrc + (size_t)k * piece_rows_bytes + (k == kmax ? srel_tail : srel0), smem + N96_SB + (k * NT + wave * 64) * 16);
        C3_T(t_issued);
#ifdef HRN_C3_TIMING
        t_pro_issue = (int)(t_issued - t_entry0);
#endif
    }
    f32x4 bias_v = f32x4{0.f, 0.f, 0.f, 0.f};   // (requested before the lane setup below, stored behind it)
    if (tid < 24) bias_v = ((const GLOBAL_AS f32x4 *)p.bias)[nt * 24 + tid];
    // (round 5: everything the first stage needs but the first LDS-DMA pieces do not -- the swizzle bits, the pixel -> slab-row map of
    // a compact tile -- is worked out HERE, while those pieces are in flight, instead of in front of them)
    // Per-lane LDS byte offset of k-group g of tap c relative to the lane's own pixel row in the slab = shift_c * 64
    // (wave-uniform) + slot * 16, slot = g ^ 2 b_c with b_c = bit 2 of (row + shift_c) (+ 16 i rows leaves bit 2 alone):
    // the nine b_c live in ONE register, the address is put together per chunk (2 VALU ops beside 6 MR MFMAs).
    unsigned swz = 0;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        const int shift = (c / 3) * p.wp + (c % 3);
        swz |= (unsigned)(((wave * 16 * MR + li + shift) >> 2) & 1) << c;
    }
    const unsigned xrow0 = lds0 + N96_SB + (wave * 16 * MR + li) * ROWB + g * 16;
    const int swz_step = (g & 2) ? -32 : 32;
    // PF: per pixel fragment, for the tile in work -- slab address of the lane's pixel (its window's first row), the nine swizzle
    // bits; CP: + the flat row of the tile's first pixel (scalar) and, from the epilogue on, the byte offsets of the parked stores
    unsigned xrow_f[PF ? MR : 1], swz_f[PF ? MR : 1], st_off[CP ? MR : 1];
    int f0_cur = 0;
    auto map_tile = [&](int t) {
        if constexpr (PF) {
            const int c0 = t * BM;
            f0_cur = tile_first(t);
#pragma unroll
            for (int i = 0; i < MR; ++i) {
                int lrow = li;
                asm volatile("" : "+v"(lrow));
                const int c = c0 + wave * 16 * MR + i * 16 + lrow;
                int rel = c - c0;
                if constexpr (CP) rel = flat_of(c < m ? c : m - 1) - f0_cur;   // (lanes past the end: the last pixel again, never stored)
                xrow_f[i] = lds0 + N96_SB + rel * ROWB + g * 16;
                unsigned sw = 0;
#pragma unroll
                for (int c9 = 0; c9 < 9; ++c9) sw |= (unsigned)(((rel + (c9 / 3) * p.wp + (c9 % 3)) >> 2) & 1) << c9;
                swz_f[i] = sw;
                asm volatile("" : "+v"(xrow_f[i]), "+v"(swz_f[i]));
            }
        }
    };
    map_tile(mt0);
    {
        if (tid < 24) *(f32x4 *)(smem + N96_BIAS + tid * 16) = bias_v;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    f32x4 acc[MR][NRB];
    s16x8 wf[NRB], xf[2][MR];
    u32x4 rpre[MR][3];   // the residual tile (requested over the two stages before the last one), then the packed results until stored
    // accumulators start at the folded-BN bias: the lane's channels sit in the LDS copy as 16-byte groups
#define N96_INIT_ACC()                                                                                              \
    {                                                                                                               \
        _Pragma("unroll") for (int j = 0; j < NRB; ++j)                                                             \
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(acc[0][j]) : "v"(bias_a), "i"(N96_CH64 ? ((j >> 1) * 32 + (j & 1) * 4) * 4 : j * 16)); \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                          \
        _Pragma("unroll") for (int i = 1; i < MR; ++i) _Pragma("unroll") for (int j = 0; j < NRB; ++j) acc[i][j] = acc[0][j]; \
    }
    N96_INIT_ACC()
    // weight fragments of stage 0, chunk 0 (what every stage leaves behind for the next one)
    {
        const unsigned wl0 = lds0 + lane * 16;
#pragma unroll
        for (int j = 0; j < NRB; ++j) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(wf[j]) : "v"(wl0), "i"(j * 1024));
    }
#ifdef N96_FAKE_BLOCKED
#define N96_PIXOFF(Q) ((unsigned)(Q) * 64u + (unsigned)(g * 16) + (unsigned)(nt * 3) * (unsigned)(fb_ss * 2))
#define N96_VOFF(V) ((unsigned)(V) * (unsigned)(fb_ss * 2))
#else
#define N96_PIXOFF(Q) (((unsigned)(Q) * (unsigned)p.cout + (unsigned)ch0) * 2u)
#define N96_VOFF(V) ((V) * VSTEP)
#endif
    // byte offset (from the tensor base; tensors are < 4 GB) of this lane's channels of pixel fragment i of M tile t.
    // (lrow opaque: formed where it is used, not carried across the loops as MR registers / 64-bit pointers)
    // CP: the flat row of the lane's pixel of fragment I of the tile IN WORK comes back out of its slab address (f0_cur + slab row);
    // a lane past the last pixel: row 0 (CLAMP: loads) or its own row of the zero tail guard behind the tensor (stores)
#define N96_ROW_OFF(T, I, CLAMP)                                                                                    \
    ({                                                                                                              \
        int lrow_ = li;                                                                                             \
        asm volatile("" : "+v"(lrow_));                                                                             \
        int qq_ = (mt0 + (T)) * BM + wave * 16 * MR + (I) * 16 + lrow_;                                             \
        if constexpr (CP) {                                                                                         \
            const int rel_ = (int)((xrow_f[PF ? (I) : 0] - (lds0 + N96_SB + g * 16)) >> 6);                         \
            qq_ = qq_ < m ? f0_cur + rel_ : ((CLAMP) ? 0 : nb * p.hpwp + (qq_ - m));                               \
        } else {                                                                                                    \
            if ((CLAMP) && qq_ >= m) qq_ = 0;                                                                       \
        }                                                                                                           \
        N96_PIXOFF(qq_);                                                                                            \
    })
    // one 16-byte store of the packed results parked in rpre (idx = 3 i + v); rows >= m land in the zero tail guard.
    // CP: the offsets were taken at the tile's epilogue (st_off) -- a parked store goes out when the NEXT tile's pixels are mapped
#define N96_STORE(T, IDX)                                                                                           \
    {                                                                                                               \
        unsigned oo_;                                                                                               \
        if constexpr (CP) oo_ = st_off[CP ? (IDX) / 3 : 0];                                                         \
        else oo_ = N96_ROW_OFF(T, (IDX) / 3, false);                                                                \
        *(GLOBAL_AS u32x4 *)((GLOBAL_AS char *)out + oo_ + N96_VOFF((IDX) % 3)) = rpre[(IDX) / 3][(IDX) % 3];      \
    }

#ifdef HRN_C3_TIMING
    int t_entry = 0, t_plan = 0, t_chunks = 0, t_ewait = 0, t_erest = 0;   // (32-bit: five SGPRs)
    C3_T(t_begin);
    const long long rt_begin = __builtin_amdgcn_s_memrealtime();   // (100 MHz: the clock the CU ran at = ticks / this)
#endif
    int q = 0;            // stage counter: weight buffer = q & 3
    // vector-memory operations this wave issued during the previous stage: np_prev LDS-DMA pieces + (kind_prev) the residual
    // loads of a last slice's stage 0 / 1 or the parked stores of a tile's first stage
    constexpr int E_R0 = NST < 6 ? NST : 6, E_R1 = NST - E_R0, E_ST = NST;
    int np_prev = 0, kind_prev = 0;   // kind: 0 none, 1 residual stage 0, 2 residual stage 1, 3 store stage
    bool st_pending = false;   // the previous tile's results are still parked in rpre
    unsigned okbits = 0;
    int slab_par = 0;
    for (int tt = 0; tt < ntile; ++tt) {
        for (int s = 0; s < S; ++s) {
            const bool has_next = !(s == S - 1 && tt == ntile - 1);
            int s2 = s + 1, t2 = tt;
            if (s2 == S) s2 = 0, ++t2;
            // the next slice's slab -> the other slab buffer (parts 0 and 1); the next slice's weights, part by part -> ring
            const long row0n = (long)tile_first(mt0 + t2) - p.wp - 1;
#ifdef N96_FAKE_BLOCKED
            const GLOBAL_AS char *const ssrc = (const GLOBAL_AS char *)(in + (row0n < 0 ? 0 : row0n) * 32 + (size_t)s2 * fb_ss);
#else
            const GLOBAL_AS char *const ssrc = (const GLOBAL_AS char *)(in + row0n * p.cin + s2 * 32);
#endif
            const unsigned sdst = lds0 + N96_SB + (slab_par ^ 1) * SLABB + wave * 1024;
            const GLOBAL_AS char *const wsrc_s = wsrc_nt + (size_t)s2 * (3 * WST) + wave * 1024;   // wave-uniform
            const bool last_slice = s == S - 1;
            // which of a stage's six LDS-DMA slots this wave fills: bits 0-2 weight pieces, bits 3-5 slab pieces (part 0 / part 1)
            const unsigned wbits = has_next ? (1u << nw_wave) - 1u : 0u;
            const unsigned sbits0 = has_next ? ((1u << ns_p0) - 1u) << 3 : 0u, sbits1 = has_next ? ((1u << ns_p1) - 1u) << 3 : 0u;
            // results parked by the previous tile's epilogue go out under this tile's first stage (S >= 2: rpre is not
            // needed again before the last slice)
            const bool st_slice = st_pending && s == 0;
#pragma unroll
            for (int P = 0; P < 3; ++P) {
                // ---- stage entry: everything this wave issued before the previous stage has landed; meet the block
                C3_T(tA);
                n96_vmcnt_dyn(np_prev + (kind_prev == 0 ? 0 : kind_prev == 1 ? E_R0 : kind_prev == 2 ? E_R1 : E_ST));
#ifndef N96_NOBARRIER   // (timing-only ablation)
                __builtin_amdgcn_s_barrier();
#endif
                const unsigned sl_a = xrow0 + slab_par * SLABB;
                if (P == 0) {   // a new slab: its pixel fragments could not be requested ahead of the barrier
                    if constexpr (PF) {
#pragma unroll
                        for (int i = 0; i < MR; ++i) {
                            unsigned sw0 = swz_f[i];
                            asm volatile("" : "+v"(sw0));
                            const unsigned xa = xrow_f[i] + slab_par * SLABB + N96_XOFF(0, sw0);
                            asm volatile("ds_read_b128 %0, %1" : "=v"(xf[0][i]) : "v"(xa));
                        }
                    } else {
                        unsigned sw0 = swz;
                        asm volatile("" : "+v"(sw0));
                        const unsigned xa = sl_a + N96_XOFF(0, sw0);
#pragma unroll
                        for (int i = 0; i < MR; ++i)
                            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xf[0][i]) : "v"(xa), "i"(i * 1024));
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                C3_T(tB);
                const bool tile_end = P == 2 && last_slice;
                const int np_now = has_next ? nw_wave + (P == 0 ? ns_p0 : P == 1 ? ns_p1 : 0) : 0;
                const unsigned dbits = wbits | (P == 0 ? sbits0 : P == 1 ? sbits1 : 0u);
                const unsigned wdst = lds0 + ((q + 3) & 3) * WST + wave * 1024;
                const GLOBAL_AS char *const wsrc = wsrc_s + P * WST;
                // the residual tile is requested over stages 0 and 1 of the last slice, one load per slot (a burst of 3 MR loads
                // per wave at one point costs the block 2-4 k cycles of vector-memory issue during which no MFMA goes out)
                // (round 6: only when there IS a residual -- conv1 of a BasicBlock used to fetch 3 MR x 1 KiB of guard-row zeros per wave
                // and tile through the same slots "for one code path": 12 vector-memory instructions whose issue the matrix pipe pays for)
#ifdef N96_RES_ALWAYS   // (A/B: round 5's behaviour)
                const bool res_stage = last_slice && P < 2;
#else
                const bool res_stage = last_slice && P < 2 && has_res;
#endif
                const bool st_stage = st_slice && P == 0;
                if (last_slice && P == 0) {
                    // the epilogue's pad mask, worked out here where the VALU work hides under the partner's MFMAs
                    okbits = 0;
#pragma unroll
                    for (int i = 0; i < MR; ++i) {
                        int lrow = li;
                        asm volatile("" : "+v"(lrow));
                        const int qq = (mt0 + tt) * BM + wave * 16 * MR + i * 16 + lrow;
                        if constexpr (CP) {   // every pixel of a compact tile is a real one
                            okbits |= qq < m ? 1u << i : 0u;
                        } else {
                            const int n_img = (int)(((unsigned long long)(unsigned)qq * p.magic_hpwp) >> p.shift_hpwp);
                            const int rem = qq - n_img * p.hpwp;
                            const int ho = (int)(((unsigned long long)(unsigned)rem * p.magic_wp) >> p.shift_wp);
                            const int wo = rem - ho * p.wp;
                            okbits |= ((qq < m) && (ho < p.h) && (wo < p.wd)) ? 1u << i : 0u;
                        }
                    }
                }
                C3_T(tC);
#if N96_TRIM
                unsigned xan[PF ? 1 : 3];   // pixel-fragment addresses of the chunks this stage pre-reads for (PF: formed per fragment at the read)
                if constexpr (!PF) {
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) {
                        unsigned sw = swz;
                        asm volatile("" : "+v"(sw));
                        xan[cc] = sl_a + N96_XOFF((3 * P + cc + 1) % 9, sw);
                    }
                }
#endif
                const unsigned wl_cur = lds0 + (q & 3) * WST + lane * 16;
                const unsigned wl_nxt = lds0 + ((q + 1) & 3) * WST + lane * 16;
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) {
                    const int xs = (3 * P + cc) & 1;                     // pixel-fragment set of this chunk
                    const bool xpre = !(P == 2 && cc == 2);              // this chunk requests the next chunk's pixels
                    const bool prev_xpre = !(P == 0 && cc == 0);         // ... and the previous one did so for this chunk
                    const unsigned wl_rd = cc == 2 ? wl_nxt : wl_cur;    // weights of the next chunk: (cc + 1) % 3 of ...
#if N96_TRIM
                    const unsigned xa_n = PF ? 0u : xan[PF ? 0 : cc];
#else
                    unsigned sw = swz;
                    asm volatile("" : "+v"(sw));
                    const unsigned xa_n = sl_a + N96_XOFF((3 * P + cc + 1) % 9, sw);
#endif
#pragma unroll
                    for (int j = 0; j < NRB; ++j) {
                        // LDS operations in issue order: behind group j, W(c+1,j) then the pixel fragments X(c+1,i) with
                        // i / N96_XPG == j.  The last of those goes out behind group JX; group 0 of the next chunk needs it (the
                        // 5 - JX weight reads behind it may still be in flight), groups j > JX need their own W(c,j), behind
                        // which 5 - j reads of the previous chunk and j + (MR) reads of this one were issued.
                        constexpr int JX = (MR - 1) / N96_XPG;
                        if (j == 0) {
                            if (prev_xpre) asm volatile("s_waitcnt lgkmcnt(%0)" ::"i"(NRB - 1 - JX) : "memory");
                        } else if (N96_TRIM ? j == JX + 1 : j > JX) {
                            // N96_TRIM: ONE wait for W(c, JX+1 .. 5): whatever this chunk issued so far may still be in flight
                            asm volatile("s_waitcnt lgkmcnt(%0)" ::"i"(N96_TRIM ? JX + 1 + (xpre ? MR : 0) : (xpre ? 5 + MR : 5)) : "memory");
                        }
                        // in-place MFMAs, written out: as builtins hipcc renames the accumulators from chunk to chunk (D != C)
                        // and needs up to twice their registers
#pragma unroll
                        for (int i = 0; i < MR; ++i)
                            if constexpr (DT == DT_F16)
                                asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc[i][j]) : "v"(wf[j]), "v"(xf[xs][i]));
                            else
                                asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[i][j]) : "v"(wf[j]), "v"(xf[xs][i]));
                        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(wf[j]) : "v"(wl_rd), "i"((((cc + 1) % 3) * NRB + j) * 1024));
                        if (xpre) {
#pragma unroll
                            for (int i = j * N96_XPG; i < (j + 1) * N96_XPG && i < MR; ++i) {
                                if constexpr (PF) {
                                    unsigned swi = swz_f[i];
                                    asm volatile("" : "+v"(swi));
                                    const unsigned xa_i = xrow_f[i] + slab_par * SLABB + N96_XOFF((3 * P + cc + 1) % 9, swi);
                                    asm volatile("ds_read_b128 %0, %1" : "=v"(xf[xs ^ 1][i]) : "v"(xa_i));
                                } else {
                                    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xf[xs ^ 1][i]) : "v"(xa_n), "i"(i * 1024));
                                }
                            }
                        }
                        // vector memory: 18 slots per stage, one operation each at most
                        const int gi = cc * NRB + j, sl = gi / 3;
                        if (gi % 3 == 1) {          // LDS-DMA: six slots, three groups (~200 MFMA cycles of the pair) apart
                            unsigned db = dbits;
                            asm volatile("" : "+s"(db));   // tested here (s_bitcmp + branch), not turned into six booleans at the stage top
                            if (db & (1u << sl)) {
                                if (sl < 3) {
                                    n96_glds(wsrc + sl * 8192, lane16, wdst + sl * 8192);
                                } else if (P < 2) {
                                    const int k = P * NSH + (sl - 3);
                                    n96_glds(ssrc + (size_t)k * piece_rows_bytes, k == kmax ? srel_tail : srel0, sdst + k * (NT * 16));
                                }
                            }
                        } else if (gi % 3 == 2) {   // residual loads (last slice, stages 0 and 1) / parked stores 6.. (first stage)
                            const int idx = P * 6 + sl;
#if !defined(N96_NOEPI)
                            if (P < 2 && idx < NST && res_stage) {
                                const unsigned ro = has_res ? N96_ROW_OFF(tt, idx / 3, true) : 0u;
#ifdef N96_FAKE_BLOCKED
                                asm volatile("global_load_dwordx4 %0, %1, %2"
                                             : "=v"(rpre[idx / 3][idx % 3])
                                             : "v"(ro + N96_VOFF(idx % 3)), "s"(res)
                                             : "memory");
#else
                                asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3"
                                             : "=v"(rpre[idx / 3][idx % 3])
                                             : "v"(ro), "s"(res), "i"((idx % 3) * VSTEP)
                                             : "memory");
#endif
                            }
#endif
                            if (P == 0 && 6 + sl < NST && st_stage) N96_STORE(tt - 1, 6 + sl)
                        } else {                    // parked stores 0..5 (first stage of the next tile)
                            if (P == 0 && sl < NST && st_stage) N96_STORE(tt - 1, sl)
                        }
                    }
                }
                C3_T(tD);
#ifdef HRN_C3_TIMING
                t_entry += (int)(tB - tA), t_plan += (int)(tC - tB), t_chunks += (int)(tD - tC);
#endif
                __builtin_amdgcn_sched_barrier(0);
                ++q;
                np_prev = np_now;
                kind_prev = res_stage ? 1 + P : st_stage ? 3 : 0;
                if (st_stage) st_pending = false;
                if (P == 2) slab_par ^= 1;
#ifdef N96_NOEPI        // (timing-only ablation)
                if (tile_end) kind_prev = 0;
                else
#endif
                if (tile_end) {
                    // ---- epilogue: (+ residual) (ReLU), zero on pad pixels.  MFMA results -> VALU readers first (the asm MFMAs are
                    // opaque to hipcc's hazard pass); the residual loads are older than this stage's pieces
                    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
                    C3_T(tE);
                    n96_vmcnt_dyn(np_now);
                    __builtin_amdgcn_sched_barrier(0);
                    C3_T(tF);
#ifndef N96_RES_ALWAYS
                    if (!has_res) {   // no residual: rpre still holds the previous tile's packed results (stored long ago)
#pragma unroll
                        for (int i = 0; i < MR; ++i)
#pragma unroll
                            for (int v = 0; v < 3; ++v) rpre[i][v] = u32x4{0u, 0u, 0u, 0u};
                    }
#endif
#pragma unroll
                    for (int i = 0; i < MR; ++i) {
                        const bool ok = (okbits >> i) & 1u;
                        const float lim = ok ? __builtin_inff() : 0.f;
                        unsigned pk[2 * NRB];
#pragma unroll
                        for (int j = 0; j < NRB; ++j) {
                            const unsigned r01 = rpre[i][j >> 1][2 * (j & 1)], r23 = rpre[i][j >> 1][2 * (j & 1) + 1];
                            float v0 = acc[i][j][0] + Tr<DT>::lo(r01);
                            float v1 = acc[i][j][1] + Tr<DT>::hi(r01);
                            float v2 = acc[i][j][2] + Tr<DT>::lo(r23);
                            float v3 = acc[i][j][3] + Tr<DT>::hi(r23);
                            if (p.relu) {
                                // ReLU and the pad mask in ONE op per value: med3(x, 0, lim), lim = +inf on real pixels, 0 on pad pixels
                                asm("v_med3_f32 %0, %1, 0, %2" : "=v"(v0) : "v"(v0), "v"(lim));
                                asm("v_med3_f32 %0, %1, 0, %2" : "=v"(v1) : "v"(v1), "v"(lim));
                                asm("v_med3_f32 %0, %1, 0, %2" : "=v"(v2) : "v"(v2), "v"(lim));
                                asm("v_med3_f32 %0, %1, 0, %2" : "=v"(v3) : "v"(v3), "v"(lim));
                                const unsigned lo = Tr<DT>::pk(v0, v1), hi = Tr<DT>::pk(v2, v3);   // RNE, v_cvt_pk_{bf16,f16}_f32
                                pk[2 * j] = lo;
                                pk[2 * j + 1] = hi;
                            } else {
                                const unsigned lo = Tr<DT>::pk(v0, v1), hi = Tr<DT>::pk(v2, v3);
                                pk[2 * j] = ok ? lo : 0u;
                                pk[2 * j + 1] = ok ? hi : 0u;
                            }
                        }
#pragma unroll
                        for (int v = 0; v < 3; ++v) rpre[i][v] = u32x4{pk[4 * v], pk[4 * v + 1], pk[4 * v + 2], pk[4 * v + 3]};
                        __builtin_amdgcn_sched_barrier(0);   // one pixel fragment at a time: 12 packed registers live, not 12 MR
                    }
                    if constexpr (CP) {
#pragma unroll
                        for (int i = 0; i < MR; ++i) st_off[i] = N96_ROW_OFF(tt, i, false);
                    }
                    if (tt + 1 < ntile && S >= 2) {
                        st_pending = true;       // stored under the next tile's first stage, one store per slot
                    } else {
#pragma unroll
                        for (int idx = 0; idx < NST; ++idx) N96_STORE(tt, idx)
                    }
                    if constexpr (CP) {          // the next tile's pixels -> slab rows (its first stage reads them)
                        if (tt + 1 < ntile) map_tile(mt0 + tt + 1);
                    }
                    N96_INIT_ACC()
#ifdef HRN_C3_TIMING
                    C3_T(tG);
                    t_ewait += (int)(tF - tE), t_erest += (int)(tG - tF);
#endif
                }
            }
        }
    }
#ifdef HRN_C3_TIMING
    if (lane == 0 && g_c3_timing) {
        C3_T(t_end);
        long long *o = g_c3_timing + ((size_t)blockIdx.x * 8 + wave) * 8;
        o[0] = (long long)t_entry | ((__builtin_amdgcn_s_memrealtime() - rt_begin) << 32), o[1] = (long long)t_plan | ((t_begin - t_entry0) << 32), o[2] = t_chunks, o[3] = (long long)t_ewait | ((long long)t_pro_issue << 32), o[4] = t_end - t_begin, o[5] = q, o[6] = 90 + MR,
        o[7] = (long long)t_erest | ((long long)ntile << 48);
    }
#endif
#undef N96_INIT_ACC
#undef N96_XOFF
#undef N96_ROW_OFF
#undef N96_STORE
#undef N96_PIXOFF
#undef N96_VOFF
}
