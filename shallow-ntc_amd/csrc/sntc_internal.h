// Internal declarations shared by the HIP translation units of libsntc_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/sntc.h"

namespace sntc {

void set_error(const std::string& msg);
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);
int zero_async(void* p, size_t bytes, hipStream_t stream);   // zero a 4-byte-aligned range on the stream with a kernel (graph-replay safe)

#define SNTC_HIP(expr)                                         \
  do {                                                         \
    hipError_t _e = (expr);                                    \
    if (_e != hipSuccess) return ::sntc::hip_fail(_e, #expr);  \
  } while (0)

// ---------------------------------------------------------------------------------------------
// Gather-GEMM: out[m, col] = sum_{t < T} sum_{c < Cin} x[src(m, t), c] * Wp[col][t*Cin + c]
//   m    = (n, qy, qx) on the macro-pixel grid [Qh, Qw]
//   src  = (n, qy*sA + offy + ty*tstep, qx*sA + offx + tx*tstep), zero outside the image
//   col  -> (oy, ox, ch) = (qy*sO + oyoff[col], qx*sO + oxoff[col], ch[col]); skipped outside
// A forward conv is one group with T = kh*kw; a stride-s transposed conv is up to four groups of
// output phases that share a tap pattern (DESIGN.md "phase-grouped transposed convolution").
// ---------------------------------------------------------------------------------------------
constexpr int kMaxGroups = 4;

// Diagnostic switches (skip global loads / LDS writes / barriers of a K loop to see what it waits on) exist only in
// builds made with -DSNTC_DIAG (make DIAG=1); in the shipped library the tests fold to `false` at compile time and no
// environment variable is read on the launch path.
#ifdef SNTC_DIAG
#define SNTC_DBG(a, bit) (((a).dbg & (bit)) != 0)
#else
#define SNTC_DBG(a, bit) false
#endif

struct GGGroup {
  const float* wp;    // [NcolPad][K], K contiguous (K padded to a multiple of 16 with zeros)
  const int* taps;    // [T]   (ty << 16) | tx
  const int* cols;    // [NcolPad] ((oyoff+128) << 24) | ((oxoff+128) << 16) | ch ; -1 = padding
  int T;              // taps: a dense th x tw grid, tap t = (t / tw, t % tw)
  int tw;             // taps per row of that grid
  int K;              // padded K
  int Ncol;           // real columns
  int ntn;            // N tiles for the launched variant
  int blk0;           // static mode: first block of this group
  size_t slab_off;    // float offset of this group's split-K slabs [ksplit][M][Ncol]
  int q0y, q0x;       // origin of this group's macro-pixel grid (phase groups whose first valid q is 1)
  int steps;          // K / 16: K stages of one tile
  int tile0;          // stream-K: tiles of the preceding groups inside one row strip
  long long unit0;    // stream-K: work units (one unit = one K stage of one tile) of the preceding groups inside one strip
};

struct GGArgs {
  const float* x;
  float* y;
  const float* bias;   // [Cout] or nullptr
  const float* res;    // epilogue operand (output shape) or nullptr
  const float* aux;    // second epilogue operand or nullptr
  unsigned x_bytes;    // size of x (< 2 GiB: 32-bit buffer offsets)
  int N, H, W, Cin;
  int Qh, Qw, M;
  int Ho, Wo, Cout;
  int sA, tstep, offy, offx, sO;
  int act, epi, pro;
  int ntm;
  int ksplit;          // static mode, >= 1: number of K ranges (blocks per tile), summed by gg_reduce_kernel
  float* slab;         // split-K partial sums (workspace) or nullptr
  // Persistent stream-K mode: `nworkers` resident workgroups share the launch's work units evenly;
  // a tile cut between workers w and w + 1 is CONTINUED, not re-summed: w publishes its accumulators (sk_slab[w],
  // sk_flags[w]), w + 1 starts its fma chains from them, so every output is the same k-ordered chain as in an unsplit tile.
  int sk;              // 0: static (one K range of one tile per block); 1: stream-K
  int nworkers;
  long long units;     // sum over groups of tiles * steps
  int tps, ups;        // tiles / units per row strip (all groups): tile order is strip-major, then group, then column tile
  float* sk_slab;      // [nworkers][256 threads * 16 TN floats], raw accumulators in register layout
  int* sk_flags;       // [nworkers], zeroed on the stream before the launch
  int* status;         // sticky per-device status word (never NULL): bit 0 = a stream-K worker gave up waiting for its neighbour's
                       // hand-off (the launch's results are invalid; sntc_conv_status reports and clears it)
  // Fused ResidualBlock tail (FUSE2 instance): after the 3x3 (this launch's groups, Cout = 96, bias / act above) the 1x1
  // 96 -> Cout2 = 192 with bias2, then `epi` with res / aux, into y [M][Cout2]
  const float* w2f;    // W2 in fragment order [2 halves][3 column tiles][12 k-quads pairs][64 lanes][4], or nullptr
  const float* bias2;
  int Cout2;
  int dma;             // 1: direct-to-LDS staging (buffer_load ... lds, four ring slots) where the instantiation exists
  int bf3;             // 1: bf16 x 3 split-precision experiment (weights packed as three bf16 planes)
  int halo;            // bf3_gemm.hip: 1 = patch staging (one activation patch per channel slab shared by its taps); needs sA == 1
                       // and every group's patch within bf3p_patch_rows_max() (set by gg_launch from the instance, as dma and bf3)
  int order;           // stream-K unit order: 1 strip-major (default), 0 column tile outermost (bf3_gemm.hip: A/B switch;
                       // gather_gemm.hip: the COLM twin of the 128 x 128 instance, single-group plans whose weights exceed an XCD's L2)
  int dbg;             // -DSNTC_DIAG builds only (SNTC_GG_DBG): 1 skip global loads, 2 skip LDS writes, 4 skip barriers,
                       // 8 skip fragment reads, 16 skip the epilogue's stores, 32 its residual loads, 64 the MFMAs, 128 the fused
                       // ResidualBlock tail's second contraction -- to see what a launch waits on; results are meaningless with any bit set
  int ngroups;
  GGGroup g[kMaxGroups];
};

// Tile variant ids (BM x BN): 1..7 -> 128 x 32*v ; 8 -> 64 x 64 ; 9 -> 128 x 128 (64 x 64 per wave) ; 10 -> 256 x 128 (fp32,
// gg_kernel); 11 -> 256 x 256, 12 -> 256 x 128, 13 -> 256 x 192 (pre-split bf16 x 3, bf3_kernel in bf3_gemm.hip)
constexpr int kNumVariants = 10;   // fp32 variants
constexpr int kMaxVariant = 13;
constexpr int kStage = 16;         // K depth of one pipeline stage
// Compile-time switches of the gather GEMM's vector loader (gather_gemm_kernel.h), for A/B builds of whole libraries
// (make EXTRA=-DSNTC_GG_TAP_STATE=0 LIB=...; compare binaries through SNTC_LIB, never a run-time switch):
//   kGGTapState  per-tap row offsets from per-tile (base, mask) and a scalar delta, instead of the per-stage multiply chain: ON
//                (the 320-column HS3 launch 615 -> 594 us, the two-stream decode step 2.426 -> 2.392 ms, profiles/gg_loader_ab.json)
//   kGGTwoSets   two staging register sets in the steady state: global loads issued two stages ahead of their LDS write: OFF --
//                measured SLOWER than the single set (the same HS3 launch 615 -> 651 us alone, 594 -> 626 us on top of the tap
//                state; the step 2.426 -> 2.570 / 2.521 ms), same bits; kept as a switch for the next look at the loads' lead
//   kGGRingSlots ring slots of the register-staged loop as compile-time constants, three stages per loop iteration: LDS addresses
//                become immediates.  Per instance through gg_const_slots (gather_gemm_kernel.h); DESIGN.md 8 has the figures
#ifndef SNTC_GG_TAP_STATE
#define SNTC_GG_TAP_STATE 1
#endif
#ifndef SNTC_GG_RING_SLOTS
#define SNTC_GG_RING_SLOTS 1
#endif
constexpr bool kGGRingSlots = SNTC_GG_RING_SLOTS != 0;
#ifndef SNTC_GG_TWO_SETS
#define SNTC_GG_TWO_SETS 0
#endif
constexpr bool kGGTapState = SNTC_GG_TAP_STATE != 0;
constexpr bool kGGTwoSets = SNTC_GG_TWO_SETS != 0;

// One compiled gather-GEMM instance (gather_gemm.hip holds the table).  schedule() in conv_plan.hip resolves a
// launch to one row; residency, tile shape, slab size, LDS and the GGArgs mode fields all come from that row.
enum GGLoad { kLoadVec, kLoadVecPro, kLoadGather };   // 16-B vector loads, the same with a prologue, dword gather (Cin % 16 != 0)
enum GGStage { kStageRing, kStageDma, kStageDeep };   // register-staged ring, direct-to-LDS, deep direct-to-LDS ring (= GGArgs::dma)
enum GGForm { kFormPlain, kFormFuse2, kFormColm, kFormBf3, kFormPresplit, kFormPresplitHalo };
struct GGInstance {
  int variant;
  GGLoad load;
  GGStage stage;
  GGForm form;         // FUSE2: fused ResidualBlock tail; COLM: column-major stream-K twin; in-loop bf16 x 3; pre-split (patch staging)
  int bm, bn, threads;
  size_t lds;          // dynamic LDS bytes
  size_t slab_floats;  // stream-K: accumulator slab of one worker's hand-off
  const void* fn;
};
const GGInstance* gg_find(int variant, GGLoad load, GGStage stage, GGForm form);   // nullptr: no such instance is compiled
int gg_init();   // fills the current device's residency table once (sets every instance's dynamic-LDS attribute)
int gg_resident(const GGInstance& inst);    // workgroups of the instance the current device keeps resident
int gg_num_cus();
int* gg_status_word();                      // device pointer of the current device's sticky status word
int gg_launch(const GGInstance& inst, const GGArgs& args, int nblocks, hipStream_t stream);
int gg_reduce_launch(const GGArgs& args, hipStream_t stream);

// ---- pre-split bf16 x 3 gather GEMM (bf3_gemm.hip): 512 threads, one workgroup per CU
constexpr int kBf3PatchRounds = 5;     // patch staging: at most 5 rounds of 512 16-B chunks = 426 rows of 96 B
constexpr int kBf3DeepRing = 3;        // weight ring slots of the patch-staging 256 x 128 instance (fragments double-buffered)
int bf3p_patch_rows_max();
const void* bf3p_kernel(int variant, bool halo);

// ---- deep-factorized prior (entropy.hip, sga.hip) ----
constexpr int kMaxW = 4;   // max hidden width
constexpr int kMaxL = 5;   // max affine layers
struct DFDesc {
  int nl;
  int w[kMaxL + 1];
  int off_m[kMaxL], off_b[kMaxL], off_f[kMaxL];
  int stride;   // floats per channel record: softplus(matrix), bias, tanh(factor) per layer
};

}  // namespace sntc

struct sntc_prior {
  int channels = 0;
  sntc::DFDesc d{};
  float* rec = nullptr;
};
