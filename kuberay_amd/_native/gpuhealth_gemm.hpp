// gpuhealth_gemm — what gpuhealth.hip (bindings) and gpuhealth_gemm.hip
// (kernels and their host code) share of the burn-in's GEMM check, and below
// that what it shares with gpuhealth_gemm_narrow.hip, gpuhealth_attn.hip,
// gpuhealth_attn128.hip, gpuhealth_attn_decode.hip and gpuhealth_moe.hip: plain
// structs and a few functions, no HIP and no pybind11 types. The files are
// separate translation units so that the GEMM kernels can be compiled with a
// switch of their own (kuberay_amd/_native/build.py) while every older kernel
// is compiled exactly as before.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace ghgemm {

constexpr uint32_t kDefaultK = 1024;
// the default M = N is the smallest multiple of 64 whose tiles give every CU
// at least this many workgroups
constexpr uint32_t kWorkgroupsPerCu = 2;

struct TileStats {
  unsigned long long mismatches;
  unsigned long long first_bad;  // row * N + col, ~0 when clean
};

// Test hook: an xor into one 16-bit element of A or B in device memory,
// between the fill and the GEMM.
struct Inject {
  bool is_a = true;
  uint32_t row = 0, col = 0, mask = 0;
};

// Test hook: an xor into one 16-bit word of the LDS of one workgroup, after
// stage `stage` of it has been staged and before its first read. tile is the
// workgroup (tile_row * tiles_n + tile_col), offset the even byte offset within
// the stage: A's 8 KiB, then B's.
struct LdsInject {
  uint32_t tile = 0, stage = 0, offset = 0, mask = 0;
};

struct FaultyTile {
  uint32_t tile_row, tile_col, key;  // key: gh::location_key of where it ran
  TileStats stats;
};

struct Result {
  int dtype = 0;
  uint32_t m = 0, n = 0, k = 0;
  uint64_t mismatches = 0;
  int64_t first_bad = -1;  // row * N + col
  float got = 0.f, expected = 0.f;
  std::vector<FaultyTile> faulty;
  int workgroups = 0, cu_total = 0, cu_seen = 0;  // cu_seen: distinct places in where[]
  double elapsed_ms = 0.0;
};

struct Dump {
  std::string a, b, c, d;
};

// On the current device. m, n, k of 0 take the default: k = kDefaultK, m = n =
// the smallest multiple of 64 that gives every CU kWorkgroupsPerCu workgroups.
// Throws std::invalid_argument for m, n or k that is no positive multiple of
// 64, k above gh::kGemmMaxK (exactness) or m, n above gh::kGemmMaxMN (a bound
// on what one call allocates), a data type other than bf16 / f16, an
// injected element outside its matrix and an LDS fault outside the tiles, the
// stages or a stage's 16 KiB; std::runtime_error for a failing HIP call. Single-shot: one fill, one GEMM launch (timed with events), one check.
Result run_gemm_exact(int dtype, int64_t m, int64_t n, int64_t k, uint32_t seed,
                      const Inject* inject = nullptr, Dump* dump = nullptr,
                      const LdsInject* lds_inject = nullptr);

// one wave's transposed LDS read of words that hold their own index: 64 x 4
std::vector<std::vector<int>> run_debug_lds_tr_dump();

// --- the narrow check: fp8 and mxfp4 (gpuhealth_gemm_narrow.hip) -----------

enum NarrowMatrix : int { NARROW_A = 0, NARROW_B = 1, NARROW_SA = 2, NARROW_SB = 3 };

// Test hook: an xor into one element of A or B (8 bits for fp8, the 4 bits of
// an e2m1 code for mxfp4) or into one scale byte of SA or SB (mxfp4 only) in
// device memory, between the fill and the GEMM. row and col count elements,
// for the scales blocks of 32 along K.
struct NarrowInject {
  int which = NARROW_A;
  uint32_t row = 0, col = 0, mask = 0;
};

struct NarrowDump {
  std::string a, b, c, d, sa, sb;  // sa and sb stay empty for fp8
};

// As run_gemm_exact, for gh::FP8 and gh::MXFP4. m and n are multiples of 64 up
// to gh::kGemmMaxMN, k a multiple of gh::narrow_stage_k(dtype) up to
// gh::narrow_max_k(dtype); 0 takes the same defaults. Throws
// std::invalid_argument for anything else, for another data type, and for an
// inject outside its matrix, with a mask wider than its element or of a scale
// with fp8.
Result run_gemm_narrow_exact(int dtype, int64_t m, int64_t n, int64_t k, uint32_t seed,
                             const NarrowInject* inject = nullptr, NarrowDump* dump = nullptr);

// One wave's ds_read_b64_tr_b8 (bits = 8, 64 x 8) or ds_read_b64_tr_b4 (bits =
// 4, 64 x 16) of 512 bytes in which lane l points at byte 8 l: for every lane
// and output element the source, as lane * elements-per-lane + element.
std::vector<std::vector<int>> run_debug_lds_tr_dump_narrow(int bits);

// --- the attention check: bf16 and f16 (gpuhealth_attn.hip) ----------------

constexpr uint32_t kAttnDefaultN = 1024;

enum AttnMatrix : int { ATTN_Q = 0, ATTN_K = 1, ATTN_V = 2 };

// Test hook: an xor into one 16-bit element of Q, K or V in device memory,
// between the fill and the launch.
struct AttnInject {
  int which = ATTN_Q;
  uint32_t row = 0, col = 0, mask = 0;
};

struct AttnDump {
  std::string q, k, v, o, m, l;
};

// Unnormalised attention forward with online softmax on the current device:
// Q is m x 64, K and V are n x 64. 0 takes the default: n = kAttnDefaultN,
// m = 64 * kWorkgroupsPerCu * (number of CUs). In the Result, k is the head
// dimension, a faulty tile is a block of 64 queries (tile_col = 0) and
// first_bad is row * gh::kAttnOutCols + col, where col 0..63 is O~, 64 is m and
// 65 is l; mismatches counts elements of all three. Throws
// std::invalid_argument for m or n that is no positive multiple of 64, m above
// gh::kAttnMaxM, n above gh::kAttnMaxN (exactness), a data type other than
// bf16 / f16 and an inject outside its matrix or with a mask wider than 16
// bits; std::runtime_error for a failing HIP call.
Result run_attn_exact(int dtype, int64_t m, int64_t n, uint32_t seed,
                      const AttnInject* inject = nullptr, AttnDump* dump = nullptr);

// One wave's v_permlane16_swap and v_permlane32_swap of vdst = lane, vsrc =
// 64 + lane: [0] and [1] are the new vdst and vsrc of the 16-lane swap, [2] and
// [3] of the 32-lane swap, 64 values each.
std::vector<std::vector<int>> run_debug_permlane_dump();

// v_exp_f32 of 0, -1, .., -126 and of -inf: 128 values
std::vector<float> run_debug_exp2_dump();

// --- the causal attention check at head dimension 128 (gpuhealth_attn128.hip) --

constexpr uint32_t kAttn128DefaultL = 1024;

// Unnormalised multi-head attention forward with online softmax on the current
// device: Q, K and V are [heads · L, 128], head h in rows h·L .. h·L + L - 1;
// with causal a query sees the keys of its head up to its own position, without
// (a debug setting) all L of them. 0 takes the default: L = kAttn128DefaultL,
// heads = what gives kWorkgroupsPerCu workgroups of L / 128 a head to every CU,
// rounded up. In the Result m is the number of heads, n is L and k the head
// dimension; a faulty tile is a workgroup (tile_row = head · L / 128 + pair,
// tile_col = 0), which computes query blocks pair and L / 64 - 1 - pair of its
// head; first_bad is row * gh::kAttn128OutCols + col over the flat rows, where
// col 0..127 is O~, 128 is m and 129 is l. The inject and the dump are those of
// run_attn_exact, rows counted flat. Throws std::invalid_argument for L that
// is no positive multiple of 128 or above gh::kAttn128MaxL (exactness), heads
// below 1, heads · L above gh::kAttn128MaxRows (a bound on what one call
// allocates), a data type other than bf16 / f16 and an inject outside its
// matrix or with a mask wider than 16 bits; std::runtime_error for a failing
// HIP call.
Result run_attn128_exact(int dtype, int64_t heads, int64_t L, bool causal, uint32_t seed,
                         const AttnInject* inject = nullptr, AttnDump* dump = nullptr);

// --- the decode attention check: paged KV, GQA, split-KV (gpuhealth_attn_decode.hip) --

constexpr uint32_t kDecodeDefaultCtx = 2048;
constexpr uint32_t kDecodeDefaultGroup = 8;
constexpr uint32_t kDecodeDefaultKvHeads = 8;
constexpr uint32_t kDecodeDefaultSplits = 4;
// the place of a faulty tile that is no workgroup: the merge over splits
constexpr uint32_t kDecodeNoCu = ~0u;

// AttnInject's fourth target: one block-table entry, row = sequence, col =
// logical page, xored with a non-zero mask below the pool size, so that the
// kernel reads a wrong page inside the pool. For ATTN_Q the row is the flat Q
// row, for ATTN_K and ATTN_V the logical row gh::decode_kv_row of an owned
// position; the host finds the slot through the clean table.
constexpr int ATTN_TABLE = 3;

struct DecodeResult : Result {
  uint32_t batch = 0, kv_heads = 0, group = 0, splits = 0, max_ctx = 0;
  uint64_t kv_bytes = 0;   // K and V rows one launch reads
  double merge_ms = 0.0;   // the merge kernel; elapsed_ms is the main kernel
};

struct DecodeDump {
  std::string q, k_pool, v_pool, table, ctx, partial, o, m, l;
};

// Unnormalised decode attention on the current device: one query token for
// each of batch sequences, kv_heads KV heads with `group` query heads each
// (1, 2, 4, 8 or 16), over a paged KV cache of 16-token pages found through a
// block table, the context of sequence b being ctx[b] in [1, max_ctx], max_ctx
// at most gh::kDecodeMaxCtx (exactness); `splits` workgroups (1 .. 32) share a
// (sequence, KV head) and a second kernel merges them. 0 takes the default:
// group = 8, kv_heads = 8, max_ctx = kDecodeDefaultCtx, splits =
// kDecodeDefaultSplits, batch = the length of ctx or, ctx being empty, what
// gives every CU kWorkgroupsPerCu workgroups; an empty ctx takes
// gh::decode_default_ctx. In the Result m is the number of Q rows, n is
// max_ctx and k the head dimension; first_bad is row * gh::kAttn128OutCols +
// col over the finals, which alone decide mismatches. A faulty tile is
// (b · kv_heads + hk, split) for a workgroup whose partial is bad, and
// (b · kv_heads + hk, splits) with key kDecodeNoCu for a KV row whose finals
// are bad while its partials are clean: the merge. Throws
// std::invalid_argument for anything outside these ranges, batch · kv_heads
// above gh::kDecodeMaxKvRows, pools above gh::kDecodeMaxPoolBytes (a bound on
// what one call allocates), a ctx list of the wrong length or with an entry
// outside [1, max_ctx], a data type other than bf16 / f16 and an inject
// outside what the check owns or with a mask that is zero, wider than 16 bits
// or, for the table, not below the pool size; std::runtime_error for a failing
// HIP call.
DecodeResult run_attn_decode_exact(int dtype, int64_t batch, int64_t kv_heads, int64_t group,
                                   int64_t max_ctx, int64_t splits,
                                   const std::vector<int64_t>& ctx, uint32_t seed,
                                   const AttnInject* inject = nullptr,
                                   DecodeDump* dump = nullptr);

// --- the MoE check: routed grouped GEMM, atomic scatter-add (gpuhealth_moe.hip) --

constexpr uint32_t kMoeDefaultExperts = 16;
constexpr uint32_t kMoeDefaultTopK = 2;
// the place of a faulty tile that is no workgroup: Y is bad over clean products
constexpr uint32_t kMoeNoCu = kDecodeNoCu;
// and of the one that stands for P's guard rows when a word of them is not zero
constexpr uint32_t kMoeGuardKey = ~0u - 2u;

enum MoeTarget : int { MOE_X = 0, MOE_W = 1, MOE_ROUTE = 2 };

// Test hook: an xor in device memory between the fill and the launch. MOE_X:
// the 16-bit element (token row, col) of X; MOE_W: element (expert · K + row,
// col) of W; MOE_ROUTE: the token id of sorted entry `row` (col 0), with a
// non-zero mask whose result stays below T, so that the kernel gathers and
// scatters a wrong token inside the batch.
struct MoeInject {
  int which = MOE_X;
  uint32_t row = 0, col = 0, mask = 0;
};

struct MoeResult : Result {
  uint32_t tokens = 0, experts = 0, top_k = 0, entries = 0;
  uint32_t tiles = 0;  // row tiles that found an expert, from where[]
};

struct MoeDump {
  std::string x, w, offsets, sorted_token, sorted_weight, p, y;
};

// The routed expert GEMM of a mixture-of-experts layer on the current device:
// X [tokens + 1, k] (the last row poison), W [experts, k, n], every token to
// top_k distinct experts with a weight in {1, 1/2, 1/4}; P [entries + 64, n]
// holds the unweighted products in sorted-entry order, Y [tokens + 1, n] the
// weighted sums, added by fp32 atomics. `route` is tokens · top_k expert ids,
// token-major, or empty for gh::moe_default_expert. 0 takes the default:
// experts = 16, top_k = 2, k = n = 1024, tokens = the length of route / top_k
// or, route being empty, the smallest multiple of 64 at which the generated
// routing gives every CU kWorkgroupsPerCu workgroups that find a tile; a shape
// that cannot do so up to gh::kMoeMaxTokens has no default and needs tokens.
// In the Result m is tokens; first_bad (row * n + col) is over Y, guard row
// included, and mismatches counts Y plus every non-zero word of P's guard
// rows; workgroups counts those that found a tile. A faulty tile is (row tile,
// column tile) for a workgroup whose rows of P are bad, (0, 0) with key
// kMoeNoCu when Y is bad while every P is clean: the scatter, and (one past
// the grid's row tiles, 0) with key kMoeGuardKey for dirty guard rows of P,
// its first_bad being row of P * n + col. Throws
// std::invalid_argument for a data type other than bf16 / f16, k or n that is
// no positive multiple of 64, k above gh::kMoeMaxK (exactness), n above
// gh::kGemmMaxMN, experts outside 1 .. 64, top_k outside 1 .. min(8, experts),
// tokens below 1, above gh::kMoeMaxTokens or needing more than
// gh::kMoeMaxBytes, a route of the wrong length, with an id out of range or
// with an expert twice in a token, and an inject outside its target, with a
// mask that is zero or wider than 16 bits or, for the route, with a result
// that is no token; std::runtime_error for a failing HIP call.
MoeResult run_moe_exact(int dtype, int64_t tokens, int64_t experts, int64_t top_k, int64_t k,
                        int64_t n, const std::vector<int64_t>& route, uint32_t seed,
                        const MoeInject* inject = nullptr, MoeDump* dump = nullptr);

}  // namespace ghgemm
