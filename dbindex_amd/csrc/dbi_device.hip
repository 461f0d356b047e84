// dbi_device.hip — CDNA4 (gfx950) kernels of the peptide-index build and the
// mass-window query.  Written for 64-wide wavefronts; compiled with
// -ffp-contract=off so the fp64 mass accumulation is the plain sequential
// left-to-right sum of DBIndexer.cutSeq (DBIndexer.java:265-308), i.e.
// bit-identical to the reference's masses.
//
// Build pipeline (one stream, dbi_engine.hip: run_digest + build_tail):
//   0. k_tile_proteins    — first/last protein of every 4096-start digest tile,
//                            longest protein (the record field width).
//   1. k_digest_bounded   — (full enzyme, mc <= 2, warm builds) per tile: window
//                            staged in LDS, cut / cleave / protein-start bit maps,
//                            cleavage-site starts compacted, each start's
//                            candidate ends from the cut map, the tile's slots
//                            reserved by one atomic add, one cutSeq mass walk per
//                            start writing 16-B records (Rec) straight into them,
//                            sentinels in the unused slots.
//      k_digest_fused     — (semi / mandatory residues / mc > 2) count walk,
//                            look-back over exact tile totals, emit walk.
//      k_digest<COUNT|EMIT> + scan — cold builds (no capacity known yet).
//   2. LSD radix passes over the fine mass bin (k_radix_hist[_u8] + scan +
//      k_radix_scatter): 3 passes of <= 8 bits at SwissProt scale; each pass
//      but the last writes the next pass's digit bytes for the next histogram;
//      record chunks are XCD-contiguous (radix_chunk) so neighbouring digit
//      runs meet in one L2.
//   3. k_chunk_bounds     — chunks of whole bins, ~CHUNK_T records each.
//   4. k_chunk_sort (<= CHUNK_CAP records, LDS, bins up to 512 records),
//      k_chunk_sort_list (chunks with a bigger bin; chunks up to BIG_CAP),
//      k_giant_* (MSD split) — sort by the 128-bit record key (mass, tag, first
//      appearance): small bins by rank, big bins by a 64-bit compact key in
//      registers (DPP bitonic, dbi_lane.h); string-verify equal (mass, tag)
//      neighbours, flag unique heads (IndexMerge.getMergedData).
//   5. scan of per-chunk unique counts, k_finalize: unique table + occurrence
//      CSR (protein ids, insertion order) + distinct mass-key count.
// Queries: k_qdir_* (query directory), k_query (range per window),
// k_hits_* (materialised hits), k_query_pairs / k_qroute_* (sharded index).
// k_hbm_copy: the measured copy ceiling the bench prints beside the peak.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <algorithm>

#include "dbi_internal.h"
#include "dbi_lane.h"

namespace dbi {

// ---------------------------------------------------------------------------
// wave / block primitives (wave = 64 lanes)
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }

__device__ __forceinline__ uint64_t lanemask_lt() {
    const unsigned l = lane_id();
    return l == 0 ? 0ull : (~0ull >> (64 - l));
}

// Orders this wave's LDS accesses before / after (a wave executes its LDS
// instructions in order; this keeps the compiler from reordering them).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        T o = __shfl_up(v, d, 64);
        if ((int)lane_id() >= d) v += o;
    }
    return v;
}

// 32-bit sums by DPP (VALU lane moves, no ds_bpermute round trips): shifts of
// 1, 2, 4, 8 inside each 16-lane row, then row 0's / rows 0-1's last lane
// broadcast into the rows above (row_bcast:15 / :31)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
}
template <>
__device__ __forceinline__ uint32_t wave_incl_scan<uint32_t>(uint32_t v) {
    v += dpp_or_zero<0x111, 0xF>(v);  // row_shr:1
    v += dpp_or_zero<0x112, 0xF>(v);  // row_shr:2
    v += dpp_or_zero<0x114, 0xF>(v);  // row_shr:4
    v += dpp_or_zero<0x118, 0xF>(v);  // row_shr:8
    v += dpp_or_zero<0x142, 0xA>(v);  // row_bcast:15 into rows 1, 3
    v += dpp_or_zero<0x143, 0xC>(v);  // row_bcast:31 into rows 2, 3
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
template <>
__device__ __forceinline__ uint32_t wave_sum<uint32_t>(uint32_t v) {
    v += lane_xor<1>(v);
    v += lane_xor<2>(v);
    v += lane_xor<4>(v);
    v += lane_xor<8>(v);
    v += lane_xor<16>(v);
    v += lane_xor<32>(v);
    return v;
}

// Block-wide exclusive scan of one value per thread.  s_tmp: >= NT/64 + 1 slots.
template <int NT, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* s_tmp, T& total) {
    constexpr int NW = NT / 64;
    const int w = threadIdx.x >> 6;
    T inc = wave_incl_scan(v);
    if (lane_id() == 63) s_tmp[w] = inc;
    __syncthreads();
    // every thread folds the (few) wave totals itself, in wave order: one
    // barrier less than a serial pass by thread 0, same additions
    T before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const T t = s_tmp[i];
        if (i < w) before += t;
        all += t;
    }
    total = all;
    __syncthreads();  // s_tmp reusable
    return inc - v + before;
}

template <int NT, typename T>
__device__ __forceinline__ T block_sum(T v, T* s_tmp) {
    T tot;
    block_excl_scan<NT, T>(v, s_tmp, tot);
    return tot;
}

__device__ __forceinline__ uint32_t bin_of(double m, const BinMap& bm) {
    double x = (m - bm.lo) * bm.scale;
    if (!(x > 0.0)) return 0u;
    if (x >= (double)(bm.nbins - 1)) return bm.nbins - 1;
    return (uint32_t)x;
}

__device__ __forceinline__ uint64_t dbits(double m) { return (uint64_t)__double_as_longlong(m); }

// a Rec loaded as 4 dwords: x,y = q0, z,w = q1
__device__ __forceinline__ uint64_t u4_q0(const uint4& r) { return ((uint64_t)r.y << 32) | r.x; }
__device__ __forceinline__ uint64_t u4_q1(const uint4& r) { return ((uint64_t)r.w << 32) | r.z; }
__device__ __forceinline__ double u4_mass(const uint4& r) { return q0_mass(u4_q0(r)); }

// 16-B loads / stores with the streaming (nontemporal) cache policy.  Only the
// copy probe uses them: on the record kernels they were no gain (chunk sort,
// finalize) or a loss (radix scatter stores 1.65 vs 1.49 ms: its digit runs
// rely on the L2 to merge partial lines)
typedef unsigned int v4u_t __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ uint4 ld16(const uint4* p) {
    if constexpr (NT) {
        const v4u_t v = __builtin_nontemporal_load(reinterpret_cast<const v4u_t*>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    } else {
        return *p;
    }
}
template <bool NT>
__device__ __forceinline__ void st16(uint4* p, const uint4& r) {
    if constexpr (NT) {
        const v4u_t v = {r.x, r.y, r.z, r.w};
        __builtin_nontemporal_store(v, reinterpret_cast<v4u_t*>(p));
    } else {
        *p = r;
    }
}

// ---------------------------------------------------------------------------
// 1/3. digest: DBIndexer.cutSeq (:237-405) + SQLiteMult.filterSequence/addSequence
// ---------------------------------------------------------------------------
constexpr int WIN_PRE = 16;  // residues staged before the tile (N-terminal context)
constexpr int WIN = WIN_PRE + DIGEST_TILE + DIGEST_HALO;
constexpr int STARTS_PER_THREAD = DIGEST_TILE / DIGEST_THREADS;

constexpr uint32_t PST_CAP = 192;  // protein starts of a tile kept in LDS (else searched in HBM)

struct DigestSmem {
    double mass[256];
    uint64_t nokm[WIN / 64 + 2];  // bit p = N_ok at window position p (protein start, or a cut at p-1)
    uint64_t cutm[WIN / 64 + 2];  // bit p = F_CUT at p            (bounded digest: slot bounds)
    uint64_t clvm[WIN / 64 + 2];  // bit p = cleave residue at p
    uint64_t stm[WIN / 64 + 2];   // bit p = a protein starts at p (incl. one past the window)
    uint32_t pst[PST_CAP];      // poff[pf .. pl+1] (protein of a start: binary search)
    alignas(16) uint16_t win[WIN + 8];  // staged window: residue | flags << 8 (F_CLEAVE F_NOCUT F_MAND F_CUT F_LAST);
                                // slack: walk_bounded reads one entry ahead without a clamp
    uint8_t flags[256];
    alignas(8) uint16_t cand[DIGEST_TILE]; // compacted candidate starts (tile-local), in order
    uint32_t tmp[DIGEST_THREADS / 64 + 1];
};
// digest_prepare's scratch bit maps live in sm.cand until the compaction
// writes it (no LDS beyond the block's 22.8 KiB: 7 blocks per CU)
constexpr int WIN_WORDS = WIN / 64 + 2;
static_assert(2 * WIN_WORDS * 8 <= DIGEST_TILE * 2, "nocut / last maps inside sm.cand");
__device__ __forceinline__ uint64_t* nocut_map(DigestSmem& sm) { return reinterpret_cast<uint64_t*>(sm.cand); }
__device__ __forceinline__ uint64_t* last_map(DigestSmem& sm) { return reinterpret_cast<uint64_t*>(sm.cand) + WIN_WORDS; }

// OR a 16-bit slice (bit b = window position p + b) into a bit map
__device__ __forceinline__ void or_slice16(uint64_t* m, uint32_t p, uint32_t v) {
    if (!v) return;
    const uint32_t w = p >> 6, sh = p & 63u;
    atomicOr(&m[w], (unsigned long long)v << sh);
    if (sh > 48) atomicOr(&m[w + 1], (unsigned long long)v >> (64 - sh));
}

// largest p in [lo, hi) with poff[p] <= x   (poff ascending)
__device__ __forceinline__ uint32_t find_le(const uint32_t* poff, uint32_t lo, uint32_t hi, uint32_t x) {
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (poff[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// tile_pf[t] = protein containing residue min(t*TILE, R-1), t in [0, ntiles];
// tile_pf[ntiles + 1 + t] = protein containing the last residue of tile t's
// staged window (t < ntiles), so a digest block starts with two independent
// loads instead of a chain of dependent ones.  One thread per protein writes
// the entries of the positions it holds (a protein shorter than a tile holds
// at most one of each kind; empty proteins hold none, which is find_le's
// answer too: the last protein whose offset is <= the position) -- no
// per-tile binary search over the offsets (20 dependent loads at SwissProt
// scale).  Threads also fold their protein's length into ctr->max_plen.
__global__ void k_tile_proteins(const uint32_t* __restrict__ poff, uint32_t n_prot, uint32_t n_res, uint32_t ntiles,
                                uint32_t* __restrict__ tile_pf, Counters* __restrict__ ctr, uint32_t* __restrict__ zero,
                                uint32_t n_zero) {
    constexpr int64_t TL = DIGEST_TILE;
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0)  // the partitioning digest's region cursors back to zero (a memset node fewer)
        for (uint32_t i = threadIdx.x; i < n_zero; i += blockDim.x) zero[i] = 0;
    uint32_t len = 0;
    if (p < n_prot) {
        const int64_t a = poff[p], e = poff[p + 1];
        len = (uint32_t)(e - a);
        if (e > a) {
            // first protein: x_t = t*TILE (t < ntiles) in [a, e); the last protein also holds R-1 (t = ntiles)
            for (int64_t t = (a + TL - 1) / TL; t * TL < e; ++t) tile_pf[t] = p;
            if (e == (int64_t)n_res) tile_pf[ntiles] = p;
            // last protein of the window: y_0 = min(WIN, R) - 1, y_t = min(t*TILE + K + 1, R) - 1 (t >= 1)
            constexpr int64_t K = TL + DIGEST_HALO - 1;
            const int64_t y0 = min((int64_t)WIN, (int64_t)n_res) - 1;
            if (y0 >= a && y0 < e) tile_pf[ntiles + 1] = p;
            int64_t t = max((int64_t)1, (a - K + TL - 1) / TL);
            if (a - K < 0) t = 1;
            for (; t < (int64_t)ntiles && t * TL + K < e; ++t)
                if (t * TL + K >= a && t * TL + K < (int64_t)n_res) tile_pf[ntiles + 1 + t] = p;
            if (e == (int64_t)n_res) {  // windows clipped at the end of the residues end in this protein
                for (int64_t u = max((int64_t)1, ((int64_t)n_res - K + TL - 1) / TL); u < (int64_t)ntiles; ++u)
                    if (u * TL + K >= (int64_t)n_res) tile_pf[ntiles + 1 + u] = p;
            }
        }
    }
    // block max, then one atomic per block that can still raise the value
    __shared__ uint32_t s_max[4];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) len = max(len, (uint32_t)__shfl_xor((int)len, d, 64));
    if (lane_id() == 0) s_max[threadIdx.x >> 6] = len;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t m = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        if (m > __hip_atomic_load(&ctr->max_plen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&ctr->max_plen, m);
    }
}

hipError_t launch_tile_proteins(const uint32_t* d_poff, uint32_t n_prot, uint32_t n_res, uint32_t* d_tile_pf,
                                Counters* d_ctr, hipStream_t s, uint32_t* d_zero, uint32_t n_zero) {
    if (n_res == 0 || n_prot == 0)
        return d_zero && n_zero ? hipMemsetAsync(d_zero, 0, sizeof(uint32_t) * n_zero, s) : hipSuccess;
    const uint32_t ntiles = (n_res + DIGEST_TILE - 1) / DIGEST_TILE;
    DBI_LAUNCH(k_tile_proteins, dim3((n_prot + 255) / 256), dim3(256), 0, s, d_poff, n_prot, n_res, ntiles,
               d_tile_pf, d_ctr, d_zero, d_zero ? n_zero : 0u);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Motif pre-pass of a sequence peptide filter (PeptideFilterBySequence:
// Matcher.find over every prefix of every walk, DBIndexer.java:309-313).
// fend[e] = length of the shortest alternative matching the residues that end
// at e, inside e's own protein; 0: none.  A walk from s is invalid from the
// first e with a match [b, e], b >= s; the shortest alternative ending at e
// has the latest b, so that test is fend[e] <= e - s + 1, exact per start.
// One tile of FE_TILE ends per block: its residues with a halo of
// PF_MAX_ATOMS - 1 before them, the protein starts inside as a bit map, and
// the class masks, all in LDS (8.6 KiB a block).
// ---------------------------------------------------------------------------
constexpr uint32_t FE_TILE = 4096;
constexpr uint32_t FE_THREADS = 256;
constexpr uint32_t FE_HALO = PF_MAX_ATOMS - 1;
constexpr uint32_t FE_WORDS = (FE_TILE + FE_HALO) / 64 + 2;

struct FendSmem {
    uint32_t mask[PF_MAX_ALTS * PF_MAX_ATOMS * 8];  // [alt][position][word]
    uint32_t len[PF_MAX_ALTS];
    uint32_t n_alt;
    unsigned long long stm[FE_WORDS];  // bit i: a protein starts at window position i
    uint8_t res[FE_TILE + FE_HALO + 1];
};

__global__ void __launch_bounds__(FE_THREADS)
k_filter_ends(const PepFilterProg* __restrict__ prog, const uint8_t* __restrict__ res,
              const uint32_t* __restrict__ poff, uint32_t n_prot, uint32_t n_res, uint8_t* __restrict__ fend) {
    __shared__ FendSmem sm;
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * FE_TILE;
    const uint32_t t_end = min(t0 + FE_TILE, n_res);
    const uint32_t w0 = t0 >= FE_HALO ? t0 - FE_HALO : 0u;
    const uint32_t nb = t_end - w0;  // <= FE_TILE + FE_HALO
    const uint32_t* __restrict__ pm = &prog->mask[0][0][0];
    for (uint32_t i = tid; i < (uint32_t)(PF_MAX_ALTS * PF_MAX_ATOMS * 8); i += FE_THREADS) sm.mask[i] = pm[i];
    if (tid < (uint32_t)PF_MAX_ALTS) sm.len[tid] = prog->len[tid];
    if (tid == 0) sm.n_alt = min(prog->n_alt, (uint32_t)PF_MAX_ALTS);
    for (uint32_t i = tid; i < nb; i += FE_THREADS) sm.res[i] = res[w0 + i];
    for (uint32_t i = tid; i < FE_WORDS; i += FE_THREADS) sm.stm[i] = 0ull;
    __syncthreads();
    // protein starts in [w0, t_end): pf = the protein holding w0 (poff[0] = 0 <= w0)
    const uint32_t pf = find_le(poff, 0, n_prot, w0);
    if (tid == 0 && poff[pf] == w0) atomicOr(&sm.stm[0], 1ull);
    for (uint32_t p = pf + 1 + tid; p < n_prot; p += FE_THREADS) {
        const uint32_t o = poff[p];
        if (o >= t_end) break;
        if (o < w0) continue;  // (offsets not ascending: device input nobody validated)
        atomicOr(&sm.stm[(o - w0) >> 6], 1ull << ((o - w0) & 63));
    }
    __syncthreads();
    const uint32_t n_alt = sm.n_alt;
    for (uint32_t i = t0 - w0 + tid; i < nb; i += FE_THREADS) {
        // residues available back to the start of this end's protein (16: more than any alternative)
        const uint32_t lo = i >= FE_HALO ? i - FE_HALO : 0u;
        const uint32_t w = lo >> 6, b = lo & 63u;
        unsigned long long v = b ? (sm.stm[w] >> b) | (sm.stm[w + 1] << (64 - b)) : sm.stm[w];
        v &= (2ull << (i - lo)) - 1ull;  // window positions lo .. i
        const uint32_t avail = v ? i - (lo + 63u - (uint32_t)__clzll((long long)v)) + 1u : (uint32_t)PF_MAX_ATOMS;
        uint32_t best = 0;
        for (uint32_t a = 0; a < n_alt; ++a) {
            const uint32_t L = sm.len[a];
            if (L == 0 || L > avail || L > i + 1 || (best && L >= best)) continue;
            bool ok = true;
            for (uint32_t k = 0; k < L && ok; ++k) {
                const uint32_t c = sm.res[i + 1 - L + k];
                ok = (sm.mask[(a * PF_MAX_ATOMS + k) * 8 + (c >> 5)] >> (c & 31u)) & 1u;
            }
            if (ok) best = L;
        }
        fend[w0 + i] = (uint8_t)best;
    }
}

hipError_t launch_filter_ends(const PepFilterProg* d_prog, const uint8_t* d_res, const uint32_t* d_poff,
                              uint32_t n_prot, uint32_t n_res, uint8_t* d_fend, hipStream_t s) {
    if (n_res == 0 || n_prot == 0) return hipSuccess;
    DBI_LAUNCH(k_filter_ends, dim3((n_res + FE_TILE - 1) / FE_TILE), dim3(FE_THREADS), 0, s, d_prog, d_res, d_poff,
               n_prot, n_res, d_fend);
    return hipGetLastError();
}

struct WalkOut {
    uint32_t kept;
    uint32_t dropped;
    bool overflow;  // the LDS window ended before the walk did: redo it from HBM
};

// One start s: the cutSeq inner loop (DBIndexer.java:256-397) in branch-light
// form over the staged window.  Per residue step: the window entry, the mass
// lookup, one fp64 add and three fp64 compares; the cleavage decision
// checkCleavage(:318) and the protein end are precomputed window flags:
//   F_CUT  = last residue of the protein, or cleave(seq[e]) && !nocut(seq[e+1])
//   F_LAST = last residue of the protein
//   SEMI  : checkCleavage = N_ok || C_ok (full mode: candidates are N_ok by
//           construction, so cut == C_ok == F_CUT)
//   MAND  : getMandatoryInternalAAs() != null (break + filterSequence path)
// Identical decisions to the literal loop: the mass is the same sequential
// fp64 sum; once m > maxMH the reference stops (a break at a cut, the while
// condition elsewhere); m <= maxMH and m >= minMH hold at every emit, so the
// non-mandatory filterSequence is always INCLUDE.
// dbi_set_windows filter: m inside one of the sorted disjoint closed intervals
// (MassRangeFilteringIndex.filterSequence :90-108 INCLUDE)
__device__ __forceinline__ bool in_windows(const DevParams& dp, double m) {
    uint32_t lo = 0, hi = dp.n_win;  // first interval starting above m
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (dp.win_lo[mid] <= m) lo = mid + 1;
        else hi = mid;
    }
    return lo > 0 && m <= dp.win_hi[lo - 1];
}

// HIST (COUNT only): every INCLUDE'd occurrence also counted in its SQLiteMult
// bucket, hist[min((int)m / BUCKET_MASS_RANGE, NUM_BUCKETS)] (LDS).
__device__ __forceinline__ void hist_add(const DevParams& dp, uint32_t* hist, double m) {
    atomicAdd(&hist[min(java_d2i(m) / dp.br, dp.nb)], 1u);
}

// FILT: a peptide filter (dbi_set_peptide_filter) ends the walk at the first
// end whose peptide is invalid, asked first in a step (DBIndexer.java:309-313);
// fend is read from HBM (L2: a byte per residue, shared by the tile's walks).
__device__ __forceinline__ bool filter_breaks(const DevParams& dp, uint32_t fl, uint32_t s, uint32_t e,
                                              uint32_t& focc) {
    if (dp.pf_kind == 1) {
        focc += (fl / F_FOCC) & 1u;
        return focc > (uint32_t)dp.pf_max;
    }
    const uint32_t fe = dp.fend[e];
    return fe != 0 && fe <= e - s + 1;
}

template <bool EMIT, bool SEMI, bool MAND, bool HIST = false, bool FILT = false>
__device__ __forceinline__ WalkOut walk_lds(const DevParams& dp, const DigestSmem& sm, uint32_t w0, uint32_t wlim,
                                            uint32_t s, bool n_ok, uint64_t loc, Rec* __restrict__ out,
                                            const Rec* out_end, uint32_t* hist = nullptr) {
    WalkOut r{0u, 0u, false};
    double m = dp.m0;                 // precMass after H2O+H+, cTerm, nTerm (:265-271)
    if (!(m <= dp.max_mh)) return r;  // while condition before the first residue (:284)
    int mc = -1;                      // intMisCleavageCount (:280)
    bool mand_excl = false;           // a mandatory residue in [s, e-1]
    const uint32_t e_min = s + (uint32_t)dp.min_len - 1;  // pepSize >= MIN_PEP_LENGTH (:331)
    const bool can_drop = dp.drop_mass <= dp.max_mh;     // uniform
    uint32_t head = 0, tail = 0;      // peptide_tag of [s, e] (EMIT only)
    if (EMIT) {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) head |= (uint32_t)(sm.win[s - w0 + k] & 0xFFu) << (8 * k);  // slack: in bounds
    }
    uint32_t kept = 0, dropped = 0;
    uint32_t e = s;
    uint32_t cur = sm.win[e - w0];
    bool ovf;
    uint32_t focc = 0;  // FILT: counted residues in [s, e]
    // single exit at the bottom: the window overflow is one more predicate
    for (;;) {
        // next window entry first: its LDS latency overlaps this step
        const uint32_t nxt = sm.win[min(e + 1, wlim - 1) - w0];
        const uint32_t c = cur & 0xFFu;
        const uint32_t fl = cur >> 8;
        if (FILT && filter_breaks(dp, fl, s, e, focc)) {      // :309-313
            ovf = false;
            break;
        }
        m = m + sm.mass[c];                                   // :306-308
        mc += (int)(fl & F_CLEAVE);                           // :314-316
        if (EMIT) tail = (tail << 8) | c;
        const bool last = (fl & F_LAST) != 0;
        ovf = !last & (e + 1 >= wlim);  // F_CUT of the window's last entry is unknown: redo from HBM
        const bool cut = SEMI ? (n_ok | ((fl & F_CUT) != 0)) : ((fl & F_CUT) != 0);  // checkCleavage (:318)
        const bool over = m > dp.max_mh;
        const bool brk = cut & ((mc > dp.max_missed) | over);                    // :322-329
        bool emit = cut & !brk & !ovf & (e >= e_min) & (m >= dp.min_mh);         // :331
        bool mbrk = false;
        if (MAND) {
            mbrk = emit & !(mand_excl | ((fl & F_MAND) != 0));  // :334-344 (break, not continue)
            emit = emit & !mbrk & (!dp.mand_filter | mand_excl); // filterSequence (:247-263)
            mand_excl = mand_excl | ((fl & F_MAND) != 0);
        }
        const bool drop = can_drop & emit & (m >= dp.drop_mass);  // bucket > NUM_BUCKETS-1 (:282-288)
        bool keep = emit & !drop;
        if (dp.filter && keep) keep = in_windows(dp, m);
        if (EMIT && keep) {
            const uint32_t tag = peptide_tag(head, tail, e - s + 1);
            Rec rec;
            rec.q0 = rec_q0(m, tag);
            rec.q1 = rec_q1(tag, loc, e - s + 1);
            if (out + kept < out_end) out[kept] = rec;
        }
        if (HIST && (keep | drop)) hist_add(dp, hist, m);
        kept += keep;
        dropped += drop;
        const bool past = m > dp.win_max;                     // SKIP_PROTEIN_START (:351-354)
        if (brk | mbrk | last | over | ovf | past) break;     // breaks + while condition (:284)
        ++e;
        cur = nxt;
    }
    r.kept = kept;
    r.dropped = dropped;
    r.overflow = ovf;
    return r;
}

// Where walk_global's records go: sink(k, m, tag, len) for its k-th kept one.
struct RecSink {  // 16-B records at out[k] (below out_end)
    Rec* __restrict__ out;
    const Rec* out_end;
    uint64_t loc;
    __device__ __forceinline__ void operator()(uint32_t k, double m, uint32_t tag, uint32_t len) const {
        Rec rec;
        rec.q0 = rec_q0(m, tag);
        rec.q1 = rec_q1(tag, loc, len);
        if (out + k < out_end) out[k] = rec;
    }
};

// The same loop reading residues from HBM (walks that run past the staged
// window, e.g. through zero-mass residues): flags from the residue tables,
// the cut from the next residue and the protein end pe.
template <bool EMIT, bool SEMI, bool MAND, bool HIST = false, typename Sink = RecSink, bool FILT = false>
__device__ WalkOut walk_global_to(const DevParams& dp, const double* __restrict__ s_mass,
                                  const uint8_t* __restrict__ s_flags, const uint8_t* __restrict__ g_res,
                                  uint32_t s, uint32_t pe, bool n_ok, const Sink& sink, uint32_t* hist = nullptr,
                                  uint32_t hist_from = 0);

template <bool EMIT, bool SEMI, bool MAND, bool HIST = false, bool FILT = false>
__device__ __forceinline__ WalkOut walk_global(const DevParams& dp, const double* __restrict__ s_mass,
                                               const uint8_t* __restrict__ s_flags, const uint8_t* __restrict__ g_res,
                                               uint32_t s, uint32_t pe, bool n_ok, uint64_t loc,
                                               Rec* __restrict__ out, const Rec* out_end, uint32_t* hist = nullptr,
                                               uint32_t hist_from = 0) {
    return walk_global_to<EMIT, SEMI, MAND, HIST, RecSink, FILT>(dp, s_mass, s_flags, g_res, s, pe, n_ok,
                                                                 RecSink{out, out_end, loc}, hist, hist_from);
}

template <bool EMIT, bool SEMI, bool MAND, bool HIST, typename Sink, bool FILT>
__device__ WalkOut walk_global_to(const DevParams& dp, const double* __restrict__ s_mass,
                                  const uint8_t* __restrict__ s_flags, const uint8_t* __restrict__ g_res,
                                  uint32_t s, uint32_t pe, bool n_ok, const Sink& sink, uint32_t* hist,
                                  uint32_t hist_from) {
    WalkOut r{0u, 0u, false};
    double m = dp.m0;
    if (!(m <= dp.max_mh)) return r;
    int mc = -1;
    bool mand_excl = false;
    uint32_t head = 0, tail = 0;
    if (EMIT)
        for (uint32_t k = 0; k < 4 && s + k < pe; ++k) head |= (uint32_t)g_res[s + k] << (8 * k);
    uint32_t kept = 0, dropped = 0;
    uint32_t focc = 0;
    for (uint32_t e = s; e < pe; ++e) {
        const uint32_t c = g_res[e];
        const uint32_t fl = s_flags[c];
        if (FILT && filter_breaks(dp, fl, s, e, focc)) break;
        m = m + s_mass[c];
        mc += (int)(fl & F_CLEAVE);
        if (EMIT) tail = (tail << 8) | c;
        const bool last = e + 1 == pe;
        const bool c_ok = last || ((fl & F_CLEAVE) && !(s_flags[g_res[e + 1]] & F_NOCUT));
        const bool cut = SEMI ? (n_ok || c_ok) : c_ok;
        const bool over = m > dp.max_mh;
        const bool brk = cut && (mc > dp.max_missed || over);
        bool emit = cut && !brk && (int)(e - s + 1) >= dp.min_len && m >= dp.min_mh;
        bool mbrk = false;
        if (MAND) {
            mbrk = emit && !(mand_excl || (fl & F_MAND));
            emit = emit && !mbrk && (!dp.mand_filter || mand_excl);
            mand_excl = mand_excl || (fl & F_MAND);
        }
        const bool drop = emit && m >= dp.drop_mass;
        const bool keep = emit && !drop && (!dp.filter || in_windows(dp, m));
        if (EMIT && keep) sink(kept, m, peptide_tag(head, tail, e - s + 1), e - s + 1);
        if (HIST && (keep || drop) && e >= hist_from) hist_add(dp, hist, m);
        kept += keep;
        dropped += drop;
        if (brk || mbrk || last || over || m > dp.win_max) break;
    }
    r.kept = kept;
    r.dropped = dropped;
    return r;
}

// One digest tile: starts [t0, t_end), staged window [w0, w_end), proteins [pf, pl].
struct TileCtx {
    uint32_t t0, t_end, w0, w_end, nbytes, pf, pl;
    uint32_t npst;  // entries of sm.pst (0: the tile's protein starts did not fit)
    uint32_t w;     // record field width (EMIT)
};

__device__ __forceinline__ bool bit_at(const uint64_t* m, uint32_t p) { return (m[p >> 6] >> (p & 63)) & 1ull; }
// bits p, p+1, ... of a bit map (bit 0 = position p)
__device__ __forceinline__ uint64_t bits_from(const uint64_t* m, uint32_t p) {
    const uint32_t w = p >> 6, b = p & 63;
    return b ? (m[w] >> b) | (m[w + 1] << (64 - b)) : m[w];
}

// N_ok(s) for tile position i: protein N-terminus, or the previous position is a cut
__device__ __forceinline__ bool n_ok_at(const DigestSmem& sm, const TileCtx& tc, uint32_t i) {
    return bit_at(sm.nokm, tc.t0 + i - tc.w0);
}

__device__ uint4 g_zero16;  // load target of lanes with nothing to load (stays zero)

// Stage the tile's window (residues + class flags + cut / protein-end flags)
// and the residue tables in LDS, and compact the candidate starts (every start
// in SEMI mode, else the N_ok ones) into sm.cand.  Returns the candidate count.
template <bool SEMI>
__device__ uint32_t digest_prepare(DigestSmem& sm, TileCtx& tc, uint32_t tile, uint32_t ntiles,
                                   const double* __restrict__ d_mass_tab,
                                   const uint8_t* __restrict__ d_flags, const uint8_t* __restrict__ d_res,
                                   const uint32_t* __restrict__ d_poff, uint32_t n_prot, uint32_t n_res,
                                   const uint32_t* __restrict__ d_tile_pf, Counters* __restrict__ d_ctr) {
    const uint32_t tid = threadIdx.x;
    tc.t0 = tile * (uint32_t)DIGEST_TILE;
    tc.t_end = min(tc.t0 + (uint32_t)DIGEST_TILE, n_res);
    tc.w0 = tc.t0 >= (uint32_t)WIN_PRE ? tc.t0 - WIN_PRE : 0u;
    tc.w_end = min(tc.w0 + (uint32_t)WIN, n_res);
    tc.nbytes = tc.w_end - tc.w0;
    const uint32_t w0 = tc.w0, w_end = tc.w_end, nbytes = tc.nbytes;

    // every independent global load first: the residue window (16-B vectors
    // over its 16-B aligned interior, bytes at the ragged ends), the tile's
    // protein range, the residue tables
    constexpr uint32_t NV = (WIN / 16 + DIGEST_THREADS - 1) / DIGEST_THREADS + 1;
    const uint32_t head = (uint32_t)((16u - ((uintptr_t)(d_res + w0) & 15u)) & 15u);  // bytes before the first vector
    const uint32_t hb = min(head, nbytes);
    const uint32_t nvec = (nbytes - hb) >> 4;
    const uint32_t tail0 = hb + (nvec << 4);
    const uint4* __restrict__ vbase = reinterpret_cast<const uint4*>(d_res + w0 + hb);
    uint4 rv[NV];
#pragma unroll
    for (uint32_t k = 0; k < NV; ++k) {
        const uint32_t i = tid + k * DIGEST_THREADS;
        rv[k] = *(i < nvec ? vbase + i : &g_zero16);  // a select, not a branch: the loads go out together
    }
    // ragged ends: thread t < 16 the head byte t, 16 <= t < 32 the tail byte t-16
    uint32_t edge = 0;
    const uint32_t epos = tid < 16 ? tid : tail0 + (tid - 16);
    const bool has_edge = tid < 16 ? tid < hb : (tid < 32 && epos < nbytes);
    edge = *(has_edge ? d_res + w0 + epos : reinterpret_cast<const uint8_t*>(&g_zero16));
    tc.pf = d_tile_pf[tile];
    tc.pl = d_tile_pf[ntiles + 1 + tile];  // proteins overlapping [t0, w_end]: [pf, pl]
    sm.mass[tid] = d_mass_tab[tid];
    sm.flags[tid] = d_flags[tid];
    if (tid < WIN_WORDS) {
        sm.stm[tid] = 0;
        sm.clvm[tid] = 0;
        nocut_map(sm)[tid] = 0;
    }
    static_assert(WIN_WORDS <= DIGEST_THREADS, "one thread per bit-map word");
    const uint32_t np_all = tc.pl - tc.pf + 2;
    __syncthreads();
    uint32_t anyf = 0;  // class flags of every residue staged (F_PTM: '[' in device input)
    // residue window -> LDS as (residue | flags << 8): a vector's 16 entries
    // leave as two 16-B LDS stores when the window is 8-entry aligned; its
    // cleave and no-cut flags as 16-bit slices of the two bit maps
#pragma unroll
    for (uint32_t k = 0; k < NV; ++k) {
        const uint32_t i = tid + k * DIGEST_THREADS;
        if (i < nvec) {
            const uint32_t wv[4] = {rv[k].x, rv[k].y, rv[k].z, rv[k].w};
            uint32_t e[16];
            uint32_t clv16 = 0, noc16 = 0;
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const uint32_t c = (wv[b >> 2] >> (8 * (b & 3))) & 0xFFu;
                const uint32_t f = sm.flags[c];
                anyf |= f;
                e[b] = c | (f << 8);
                clv16 |= (f & F_CLEAVE) << b;
                noc16 |= ((f >> 1) & 1u) << b;
            }
            static_assert(F_CLEAVE == 1 && F_NOCUT == 2, "flag bits");
            or_slice16(sm.clvm, hb + i * 16, clv16);
            or_slice16(nocut_map(sm), hb + i * 16, noc16);
            if ((hb & 7u) == 0) {
                uint4* dst = reinterpret_cast<uint4*>(&sm.win[hb + i * 16]);
                dst[0] = make_uint4(e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16, e[6] | e[7] << 16);
                dst[1] = make_uint4(e[8] | e[9] << 16, e[10] | e[11] << 16, e[12] | e[13] << 16, e[14] | e[15] << 16);
            } else {
#pragma unroll
                for (int b = 0; b < 16; ++b) sm.win[hb + i * 16 + b] = (uint16_t)e[b];
            }
        }
    }
    if (has_edge) {
        const uint32_t f = sm.flags[edge];
        anyf |= f;
        sm.win[epos] = (uint16_t)(edge | (f << 8));
        or_slice16(sm.clvm, epos, f & F_CLEAVE);
        or_slice16(nocut_map(sm), epos, (f >> 1) & 1u);
    }
    if (anyf & F_PTM) atomicOr(&d_ctr->err, ERR_PTM);
    tc.npst = np_all <= PST_CAP ? np_all : 0u;
    for (uint32_t i = tid; i < np_all; i += DIGEST_THREADS) {
        const uint32_t o = d_poff[tc.pf + i];
        if (o >= w0 && o <= w_end) atomicOr(&sm.stm[(o - w0) >> 6], 1ull << ((o - w0) & 63));  // protein starts (and the end of the last one)
        if (i < PST_CAP) sm.pst[i] = o;
    }
    __syncthreads();
    // cleavage-cut and protein-end flags of every window position, and the
    // N_ok bit map (a protein start, or a cut just before: the candidate
    // starts of a full enzyme), 64 positions per thread from the bit maps:
    //   last     = a protein starts at p+1          (stm >> 1)
    //   cut      = last || (cleave(p) && !nocut(p+1))
    //   cut_prev = cleave(p-1) && !nocut(p)          (its protein-end case is a start)
    //   N_ok     = start(p) || cut_prev
    // At the window's last position (w_end < R) the next residue is unknown
    // (no no-cut bit): a walk that reaches it without a protein end
    // overflows to walk_global first.
    if (tid < WIN_WORDS) {
        const uint32_t w = tid;
        const uint64_t valid = nbytes >= 64 * w + 64 ? ~0ull
                             : nbytes <= 64 * w  ? 0ull : ((1ull << (nbytes - 64 * w)) - 1);
        const uint64_t* noc = nocut_map(sm);
        const uint64_t st = sm.stm[w];
        const uint64_t st_n = w + 1 < (uint32_t)WIN_WORDS ? sm.stm[w + 1] : 0ull;
        const uint64_t cl = sm.clvm[w];
        const uint64_t cl_p = w > 0 ? sm.clvm[w - 1] : 0ull;
        const uint64_t nc = noc[w];
        const uint64_t nc_n = w + 1 < (uint32_t)WIN_WORDS ? noc[w + 1] : 0ull;
        const uint64_t last = ((st >> 1) | (st_n << 63)) & valid;
        const uint64_t cut = (last | (cl & ~((nc >> 1) | (nc_n << 63)))) & valid;
        const uint64_t cut_prev = ((cl << 1) | (cl_p >> 63)) & ~nc;
        sm.cutm[w] = cut;
        sm.nokm[w] = (st | cut_prev) & valid;
        last_map(sm)[w] = last;
    }
    __syncthreads();
    // F_CUT / F_LAST into the window entries, 16 aligned entries per step
    {
        static_assert(F_CUT == 8 && F_LAST == 16, "cut / last bits 11, 12 of an entry");
        const uint16_t* cut16 = reinterpret_cast<const uint16_t*>(sm.cutm);
        const uint16_t* last16 = reinterpret_cast<const uint16_t*>(last_map(sm));
        for (uint32_t j = tid; j * 16 < nbytes; j += DIGEST_THREADS) {
            const uint32_t cu = cut16[j], la = last16[j];
            if ((cu | la) == 0) continue;
            uint4* src = reinterpret_cast<uint4*>(&sm.win[j * 16]);
            uint4 v[2] = {src[0], src[1]};
            uint32_t* d = reinterpret_cast<uint32_t*>(v);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint32_t c2 = (cu >> (2 * q)) & 3u, l2 = (la >> (2 * q)) & 3u;
                d[q] |= ((c2 & 1u) << 11) | ((l2 & 1u) << 12) | ((c2 >> 1) << 27) | ((l2 >> 1) << 28);
            }
            src[0] = v[0];
            src[1] = v[1];
        }
    }
    __syncthreads();
    // cleavage-site compaction: thread t owns starts [t*SPT, t*SPT+SPT) in order
    static_assert(STARTS_PER_THREAD == 16 && WIN_PRE % 16 == 0, "16-bit slices of the N_ok map");
    const uint32_t off = tc.t0 - w0;  // window position of start 0 (0 or WIN_PRE)
    const uint32_t p0 = off + tid * STARTS_PER_THREAD;
    const uint32_t n_here = tc.t0 + tid * STARTS_PER_THREAD < tc.t_end
                                ? min((uint32_t)STARTS_PER_THREAD, tc.t_end - tc.t0 - tid * STARTS_PER_THREAD) : 0u;
    const uint32_t valid = n_here >= 16 ? 0xFFFFu : ((1u << n_here) - 1u);
    uint32_t mybits = SEMI ? valid : ((uint32_t)(sm.nokm[p0 / 64] >> (p0 % 64)) & valid);
    uint32_t mycnt = (uint32_t)__popc(mybits);
    uint32_t ncand;
    uint32_t pos = block_excl_scan<DIGEST_THREADS, uint32_t>(mycnt, sm.tmp, ncand);
#pragma unroll
    for (int k = 0; k < STARTS_PER_THREAD; ++k)
        if (mybits & (1u << k)) sm.cand[pos++] = (uint16_t)(tid * STARTS_PER_THREAD + k);
    __syncthreads();
    return ncand;
}

// Protein of start s in the tile: largest p in [pf, pl] with poff[p] <= s
// (LDS copy of the tile's offsets; HBM when they did not fit), and its start.
__device__ __forceinline__ uint32_t tile_protein(const DigestSmem& sm, const TileCtx& tc,
                                                 const uint32_t* __restrict__ d_poff, uint32_t s, uint32_t& pstart) {
    if (tc.npst) {
        uint32_t lo = 0, hi = tc.npst - 1;  // pst[hi] = poff[pl+1] > s
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (sm.pst[mid] <= s) lo = mid; else hi = mid;
        }
        pstart = sm.pst[lo];
        return tc.pf + lo;
    }
    const uint32_t p = find_le(d_poff, tc.pf, tc.pl + 1, s);
    pstart = d_poff[p];
    return p;
}

// One candidate: LDS walk, or the HBM walk when it outruns the window
template <bool EMIT, bool SEMI, bool MAND, bool HIST = false, bool FILT = false>
__device__ __forceinline__ WalkOut walk_candidate(const DevParams& dp, const DigestSmem& sm, const TileCtx& tc,
                                                  const uint8_t* __restrict__ d_res,
                                                  const uint32_t* __restrict__ d_poff, uint32_t j,
                                                  Rec* __restrict__ o, const Rec* o_end, uint32_t* hist = nullptr) {
    const uint32_t i = sm.cand[j];
    const uint32_t s = tc.t0 + i;
    const bool n_ok = SEMI ? n_ok_at(sm, tc, i) : true;
    uint64_t loc = 0;
    if (EMIT) {
        uint32_t pstart;
        const uint32_t p = tile_protein(sm, tc, d_poff, s, pstart);
        loc = rec_loc(p, s - pstart, tc.w);
    }
    WalkOut w = walk_lds<EMIT, SEMI, MAND, HIST, FILT>(dp, sm, tc.w0, tc.w_end, s, n_ok, loc, o, o_end, hist);
    if (w.overflow) {  // (HIST: the LDS walk counted the ends before w_end - 1, the same as the HBM walk's)
        const uint32_t pe = d_poff[find_le(d_poff, tc.pf, tc.pl + 1, s) + 1];
        w = walk_global<EMIT, SEMI, MAND, HIST, FILT>(dp, sm.mass, sm.flags, d_res, s, pe, n_ok, loc, o, o_end, hist,
                                                      tc.w_end - 1);
    }
    return w;
}

// thread t walks candidates [jb, je): a contiguous, balanced share (thread
// order == start order, so EMIT writes land in insertion order)
__device__ __forceinline__ void thread_share(uint32_t ncand, uint32_t& jb, uint32_t& je) {
    const uint32_t q = ncand / DIGEST_THREADS, rr = ncand % DIGEST_THREADS;
    jb = threadIdx.x * q + min(threadIdx.x, rr);
    je = jb + q + (threadIdx.x < rr ? 1u : 0u);
}

// per-thread kept counts -> d_thr, per-tile totals -> d_blk, dropped -> counter
__device__ __forceinline__ void publish_counts(DigestSmem& sm, uint32_t kept, uint32_t dropped,
                                               uint32_t* __restrict__ d_blk, uint32_t* __restrict__ d_thr,
                                               Counters* __restrict__ d_ctr) {
    d_thr[blockIdx.x * DIGEST_THREADS + threadIdx.x] = kept;
    const uint32_t tk = block_sum<DIGEST_THREADS, uint32_t>(kept, sm.tmp);
    const uint32_t td = block_sum<DIGEST_THREADS, uint32_t>(dropped, sm.tmp);
    if (threadIdx.x == 0) {
        d_blk[blockIdx.x] = tk;
        if (td) atomicAdd(&d_ctr->n_dropped, (unsigned long long)td);
    }
}

// COUNT: per-thread kept counts -> d_thr, per-tile totals -> d_blk.
// EMIT : d_blk holds the exclusive per-tile offsets; a block scan of the
//        per-thread counts places each thread's contiguous run of candidates:
//        thread order == start order, so records land in insertion order.
// The block's bucket counts (HIST) into the device histogram (one atomic per
// non-empty bucket).
__device__ __forceinline__ void hist_flush(const DevParams& dp, const uint32_t* s_hist,
                                           unsigned long long* __restrict__ d_hist) {
    __syncthreads();
    for (uint32_t b = threadIdx.x; b <= (uint32_t)dp.nb; b += blockDim.x)
        if (s_hist[b]) atomicAdd(&d_hist[b], (unsigned long long)s_hist[b]);
}

template <bool EMIT, bool SEMI, bool MAND, bool HIST = false, bool FILT = false>
__global__ void __launch_bounds__(DIGEST_THREADS)
k_digest(DevParams dp, const double* __restrict__ d_mass_tab, const uint8_t* __restrict__ d_flags,
         const uint8_t* __restrict__ d_res, const uint32_t* __restrict__ d_poff, uint32_t n_prot,
         uint32_t n_res, const uint32_t* __restrict__ d_tile_pf, uint32_t* __restrict__ d_blk,
         uint32_t* __restrict__ d_thr, Rec* __restrict__ d_out, Counters* __restrict__ d_ctr,
         unsigned long long* __restrict__ d_hist = nullptr) {
    __shared__ DigestSmem sm;
    __shared__ uint32_t s_hist[HIST ? HIST_MAX_BUCKETS + 1 : 1];
    TileCtx tc;
    if (HIST)  // (digest_prepare's barriers come before the first count)
        for (uint32_t b = threadIdx.x; b <= (uint32_t)dp.nb; b += DIGEST_THREADS) s_hist[b] = 0;
    const uint32_t ncand = digest_prepare<SEMI>(sm, tc, blockIdx.x, gridDim.x, d_mass_tab, d_flags, d_res, d_poff, n_prot, n_res,
                                                d_tile_pf, d_ctr);
    uint32_t jb, je;
    thread_share(ncand, jb, je);
    if (!EMIT) {
        uint32_t kept = 0, dropped = 0;
        for (uint32_t j = jb; j < je; ++j) {
            const WalkOut w = walk_candidate<false, SEMI, MAND, HIST, FILT>(dp, sm, tc, d_res, d_poff, j, nullptr,
                                                                            nullptr, s_hist);
            kept += w.kept;
            dropped += w.dropped;
        }
        publish_counts(sm, kept, dropped, d_blk, d_thr, d_ctr);
        if (HIST) hist_flush(dp, s_hist, d_hist);
        return;
    }
    tc.w = rec_width(d_ctr->max_plen);
    if (blockIdx.x == 0 && threadIdx.x == 0 && !rec_layout_ok(tc.w, n_prot)) atomicOr(&d_ctr->err, ERR_LAYOUT);
    uint32_t tot;
    const uint32_t my = d_thr[blockIdx.x * DIGEST_THREADS + threadIdx.x];
    Rec* out = d_out + d_blk[blockIdx.x] + block_excl_scan<DIGEST_THREADS, uint32_t>(my, sm.tmp, tot);
    const Rec* out_end = reinterpret_cast<const Rec*>(~(uintptr_t)0 & ~(uintptr_t)15);  // sized from the count pass
    for (uint32_t j = jb; j < je; ++j)
        out += walk_candidate<true, SEMI, MAND, false, FILT>(dp, sm, tc, d_res, d_poff, j, out, out_end).kept;
}


// ---------------------------------------------------------------------------
// COUNT for full-enzyme digestion without mandatory residues.  Decisions only
// happen at cuts and every limit is monotone along a walk (the mass only
// grows; intMisCleavageCount only grows), so the peptides of a start are the
// cuts e in [lo, hi]: hi = min(protein end, the position before the
// (max_missed+2)-th cleave residue, the last position with m <= maxMH), lo =
// max(start + MIN_PEP_LENGTH - 1, the first position with m >= minMH).  Over
// a 64-position horizon the cut / cleave / protein-start bit maps of the
// staged window give the first two by bit selects, window-local prefix masses
// the mass limits by binary search, and a popcount the count: ~15 LDS reads
// per start instead of one step per residue (non-specific 6-50: ~40).  A
// start whose approximate mass lies within CUT_EPS Da of minMH / maxMH / the
// bucket-drop mass at a boundary, or whose walk may leave the horizon, is
// recounted by the exact walk, so the counts equal the emit pass's exactly.
// (Prefix error over a window < 3e-7 Da.)
// ---------------------------------------------------------------------------
// Window prefix masses in fixed point: p[i] = round(prefix of window
// positions [0, i] x 2^9) as u32 (residue masses < 1024 Da, DevParams::
// cut_count: a window's prefix < 4.5e6 Da < 2^32 / 512).  A peptide's mass
// m0 + P(e) - P(s-1) compares with a limit X as the integer D = p[e] - p[s-1]
// against T = floor((X - m0) x 2^9): |D - 512 (P(e) - P(s-1))| <= 1 (two
// roundings; the fp64 sums behind them are exact to ~1e-9 Da), so D >= T + 3
// is surely m >= X + 2^-9 and D <= T - 3 surely m < X; in between (within
// ~0.006 Da of a limit: ~1e-4 of the starts) the start is recounted by the
// exact walk.  One u32 LDS read per probe, integer compares.
constexpr int64_t CUT_EPS_FX = 3;
constexpr double CUT_SCALE = 512.0;

// Stored with one pad word per 32 entries: the threads of a wave own
// consecutive 16-start runs, so unpadded their reads p[ps + e] fell 16 words
// apart -- two banks for 32 lanes (SQ: ~7 bank conflicts per LDS instruction
// in the bucket count, 4.5 in the plain one).
struct CutSmem {
    uint32_t raw[WIN + 4 + (WIN + 4) / 32 + 1];  // (+ slack: the bucket count reads up to p[q + 2] unclamped)
    __device__ __forceinline__ uint32_t& p(uint32_t i) { return raw[i + (i >> 5)]; }
    __device__ __forceinline__ uint32_t p(uint32_t i) const { return raw[i + (i >> 5)]; }
};

// T of a limit X (clamped: an infinite or huge limit is never reached)
__host__ __device__ __forceinline__ int64_t cut_threshold(double x, double m0) {
    const double t = floor((x - m0) * CUT_SCALE);
    return t < -1e15 ? (int64_t)-1e15 : t > 1e15 ? (int64_t)1e15 : (int64_t)t;
}

// +1: surely m >= X; -1: surely m < X; 0: too close to tell
__device__ __forceinline__ int cut_cmp(int64_t d, int64_t t) {
    return d >= t + CUT_EPS_FX ? 1 : d <= t - CUT_EPS_FX ? -1 : 0;
}

// the limits of a count kernel, in window-prefix units
struct CutLimits {
    int64_t t_min, t_max, t_drop;
    int64_t t_b[8];  // bucket boundaries (k + 1) x BUCKET_MASS_RANGE, k < min(NUM_BUCKETS, 8)
};

__device__ __forceinline__ CutLimits cut_limits(const DevParams& dp) {
    CutLimits cl;
    cl.t_min = cut_threshold(dp.min_mh, dp.m0);
    cl.t_max = cut_threshold(dp.max_mh, dp.m0);
    cl.t_drop = cut_threshold(dp.drop_mass, dp.m0);
#pragma unroll
    for (int k = 0; k < 8; ++k) cl.t_b[k] = cut_threshold((double)((k + 1) * dp.br), dp.m0);
    return cl;
}

struct CutCount {
    uint32_t kept, dropped;
    bool exact;  // false: recount with the residue walk
};

// position of the k-th (1-based) set bit of v, 64 when v has fewer
__device__ __forceinline__ uint32_t select_bit(uint64_t v, uint32_t k) {
    if ((uint32_t)__popcll(v) < k) return 64u;
    uint32_t p = 0;
#pragma unroll
    for (uint32_t w = 32; w; w >>= 1) {
        const uint32_t c = (uint32_t)__popcll(v & ((1ull << w) - 1));
        if (c < k) {
            k -= c;
            v >>= w;
            p += w;
        }
    }
    return p;
}

// bits lo..hi (lo <= hi <= 63)
__device__ __forceinline__ uint64_t bit_range(uint32_t lo, uint32_t hi) {
    return ((2ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
}

// Bucket counts of one thread's starts (ascending) when NUM_BUCKETS <= 8: the
// per-thread counts in registers, and for every bucket boundary a merge
// pointer -- the first window position whose prefix passes it for the current
// start (p[q] > p[s-1] + T_k), over the whole window, not only the start's
// ends.  That position only moves forward from one start to the next (the
// threshold grows with the start's prefix), about one residue per start, so
// it is advanced (hist_advance) at every start, ends or not, with the prefixes
// at it and before it kept in registers.  Boundaries that no
// kept end can pass (above maxMH) or that every kept end passes (below minMH)
// are settled for the whole kernel: [k0, k1) is wave-uniform.
constexpr int HIST_FAST_MAX = 8;
// Tracked boundary i (i < KT, the kernel's compile-time count) is boundary
// k0 + i: a kernel per KT, so the per-start loops hold no disabled
// iterations and index registers statically (KT = k1 - k0, launch_digest).
struct HistTrack {
    uint32_t q[HIST_FAST_MAX];   // the boundary's pointer (0: not yet placed; T_k > any residue: never 0 once placed)
    uint32_t v[HIST_FAST_MAX];   // p[q]
    uint32_t pv[HIST_FAST_MAX];  // p[q - 1]
    uint32_t t[HIST_FAST_MAX];   // T of tracked boundary i (= CutLimits::t_b[k0 + i])
    uint32_t c[HIST_FAST_MAX + 1];  // c[i]: ends at or past tracked boundary i; c[8]: ends
    uint32_t k0, k1;  // boundaries below k0: every kept end past them; from k1 on: none
};

// first q in [t, hi + 1] with p[q] > a (p non-decreasing): gallop, then bisect
__device__ __forceinline__ uint32_t prefix_seek(const CutSmem& cs, uint32_t t, uint32_t hi, int64_t a) {
    if (t > hi || (int64_t)cs.p(t) > a) return t;
    uint32_t lo = t, step = 1;  // p[lo] <= a
    while (lo + step <= hi && (int64_t)cs.p(lo + step) <= a) {
        lo += step;
        step <<= 1;
    }
    uint32_t up = min(lo + step, hi + 1);  // p[up] > a, or up = hi + 1
    while (up - lo > 1) {
        const uint32_t mid = (lo + up) >> 1;
        if ((int64_t)cs.p(mid) > a) up = mid; else lo = mid;
    }
    return up;
}

// Every start, in order: each tracked boundary's pointer -- the first window
// position q with p[q] > p[s-1] + T_k -- moved to this start's threshold.
// The threshold grows by one residue's mass per start, so the pointer moves a
// step or two: the next three prefixes of every pointer are read in one LDS
// round trip and the pointer advanced branch-free (more than three steps
// need three residues lighter than the one the threshold grew by, or a start
// skipped: a gallop then).  The prefixes at the pointer and before it stay
// in registers.  The slack words past the window read as above every
// threshold, so no pointer passes p[nbytes].
template <int KT>
__device__ __forceinline__ void hist_advance(const CutSmem& cs, uint32_t nbytes, uint32_t upb, uint32_t ps,
                                             HistTrack& ht) {
    uint32_t w1[HIST_FAST_MAX], w2[HIST_FAST_MAX], w3[HIST_FAST_MAX];
#pragma unroll
    for (int i = 0; i < KT; ++i) {
        if (ht.q[i] == 0u || ht.q[i] < ps) {  // first start
            const uint32_t q = prefix_seek(cs, ps, nbytes - 1u, (int64_t)(upb + ht.t[i]));
            ht.q[i] = q;
            ht.v[i] = cs.p(q);
            ht.pv[i] = q > 0u ? cs.p(q - 1u) : 0u;  // (q >= ps; p[q - 1] <= the threshold)
        }
    }
#pragma unroll
    for (int i = 0; i < KT; ++i) {
        const uint32_t q = min(ht.q[i], nbytes);
        w1[i] = cs.p(q + 1u);
        w2[i] = cs.p(q + 2u);
        w3[i] = cs.p(q + 3u);
    }
    bool more = false;
#pragma unroll
    for (int i = 0; i < KT; ++i) {
        const uint32_t athr = upb + ht.t[i];
        const uint32_t q = ht.q[i], v = ht.v[i], pv = ht.pv[i];
        const bool a0 = v <= athr, a1 = a0 && w1[i] <= athr, a2 = a1 && w2[i] <= athr;
        more |= a2 && w3[i] <= athr;
        ht.q[i] = q + (uint32_t)a0 + (uint32_t)a1 + (uint32_t)a2;
        ht.pv[i] = a2 ? w2[i] : a1 ? w1[i] : a0 ? v : pv;
        ht.v[i] = a2 ? w3[i] : a1 ? w2[i] : a0 ? w1[i] : v;
    }
    if (more) {
#pragma unroll
        for (int i = 0; i < KT; ++i) {
            const uint32_t athr = upb + ht.t[i];
            if (ht.v[i] <= athr) {
                const uint32_t q = prefix_seek(cs, ht.q[i], nbytes - 1u, (int64_t)athr);
                ht.q[i] = q;
                ht.v[i] = cs.p(q);
                ht.pv[i] = cs.p(q - 1u);
            }
        }
    }
}

// first e in [a, b] with D(e) > t (D non-decreasing; b + 1 when none)
template <typename DF>
__device__ __forceinline__ uint32_t first_above(DF D, uint32_t a, uint32_t b, int64_t t) {
    uint32_t lo = a, hi = b + 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (D(mid) > t) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// HIST: the ends' SQLiteMult buckets as well -- ht (NUM_BUCKETS <= 8): the
// tracked boundaries above, counts in registers; otherwise the boundaries
// k * BUCKET_MASS_RANGE located by binary search like the limits above,
// counts into the LDS hist.  An end too close to a boundary (or more than 7
// boundaries in one walk, binary-search path) and the start is recounted by
// the exact walk.
// FAST (a kernel of its own: the binary-search path's code is not in it)
template <bool HIST = false, bool FAST = false, int KT = 0>
__device__ __forceinline__ CutCount count_by_masks(const DevParams& dp, const CutLimits& cl, const DigestSmem& sm,
                                                   const CutSmem& cs, uint32_t nbytes, uint32_t ps, uint32_t* hist,
                                                   HistTrack& ht) {
    CutCount r{0u, 0u, true};
    if (!(dp.m0 <= dp.max_mh)) return r;  // while condition before the first residue (:284)
    if (ps + 2 > nbytes) { r.exact = false; return r; }
    const int64_t pb = ps > 0 ? (int64_t)cs.p(ps - 1) : 0;
    if constexpr (HIST && FAST) hist_advance<KT>(cs, nbytes, (uint32_t)pb, ps, ht);  // every start: pointers in step
    // horizon: relative positions 0..h (the window's last position, whose cut is unknown, excluded)
    const uint32_t h = min(63u, nbytes - 2 - ps);
    const uint64_t hmask = bit_range(0, h);
    const uint64_t C = bits_from(sm.cutm, ps) & hmask;   // cuts (checkCleavage, incl. protein ends)
    const uint64_t V = bits_from(sm.clvm, ps) & hmask;   // cleave residues (intMisCleavageCount)
    const uint64_t S = bits_from(sm.stm, ps + 1) & hmask;  // bit k: the next protein starts at ps+1+k
    uint32_t H = h;
    bool ends = false;  // the walk emits nothing past H
    if (S) { H = (uint32_t)__ffsll((long long)S) - 1; ends = true; }  // protein end (:284 end < length)
    // mc > max_missed at cuts from here (:322): the (maxMC+2)-th cleave residue;
    // a horizon of cleave residues only (non-specific digests): its position
    // directly, no bit select
    const uint32_t kmc = (uint32_t)dp.max_missed + 2u;
    uint32_t xk;
    if (V == hmask) xk = kmc <= h + 1u ? kmc - 1u : 64u;
    else xk = select_bit(V, kmc);
    if (xk <= H) {  // xk >= 1
        H = xk - 1;
        ends = true;
    }
    auto D = [&](uint32_t e) -> int64_t { return (int64_t)cs.p(ps + e) - pb; };
    // last position with m <= maxMH (the walk stops past it: :284, :326)
    int Y;
    {
        const int c = cut_cmp(D(H), cl.t_max);
        if (c == 0) { r.exact = false; return r; }
        if (c < 0) {
            if (!ends) { r.exact = false; return r; }
            Y = (int)H;
        } else {
            const uint32_t a = first_above(D, 0u, H, cl.t_max);  // first e with m > maxMH
            if (cut_cmp(D(a), cl.t_max) <= 0 || (a > 0 && cut_cmp(D(a - 1), cl.t_max) >= 0)) {
                r.exact = false;
                return r;
            }
            Y = (int)a - 1;
        }
    }
    // first emittable position: pepSize >= MIN_PEP_LENGTH and m >= minMH (:331)
    int lo = dp.min_len - 1;
    if (Y < lo) return r;
    {
        const int c = cut_cmp(D((uint32_t)lo), cl.t_min);
        if (c == 0) { r.exact = false; return r; }
        if (c < 0) {
            const int cy = cut_cmp(D((uint32_t)Y), cl.t_min);
            if (cy == 0) { r.exact = false; return r; }
            if (cy < 0) return r;
            const uint32_t a = first_above(D, (uint32_t)lo + 1, (uint32_t)Y, cl.t_min);
            if (cut_cmp(D(a), cl.t_min) <= 0 || cut_cmp(D(a - 1), cl.t_min) >= 0) { r.exact = false; return r; }
            lo = (int)a;
        }
    }
    const uint64_t em = C & bit_range((uint32_t)lo, (uint32_t)Y);
    const uint32_t n = (uint32_t)__popcll(em);
    uint32_t nd = 0;
    if (dp.drop_mass <= dp.max_mh && n) {  // bucket > NUM_BUCKETS-1 (:282-288): the cuts from m >= drop_mass on
        const int cy = cut_cmp(D((uint32_t)Y), cl.t_drop), cl0 = cut_cmp(D((uint32_t)lo), cl.t_drop);
        if (cy == 0 || cl0 == 0) { r.exact = false; return r; }
        if (cy > 0) {
            const uint32_t a = first_above(D, (uint32_t)lo, (uint32_t)Y, cl.t_drop);
            if (cut_cmp(D(a), cl.t_drop) <= 0 || (a > 0 && cut_cmp(D(a - 1), cl.t_drop) >= 0)) {
                r.exact = false;
                return r;
            }
            nd = (uint32_t)__popcll(em & bit_range(a, (uint32_t)Y));
        }
    }
    if constexpr (HIST && FAST) {
      if (n) {
        // absolute window positions of the first / last end; end q is past
        // boundary k when p[q] > pb + T_k, and the pointer (hist_advance) is
        // the first such position: the ends from it on are past (u32
        // arithmetic; fast: 3 <= T_k < 2^31, a window's prefix + T_k < 2^32).
        // ht.c[k] (k < 8) sums G_k, the ends at or past boundary k; ht.c[8]
        // sums n (the bucket counts are their differences, at the flush).  An
        // end within CUT_EPS of a boundary: the start is recounted by the
        // exact walk (its counts here are never added).  Past qhi + 1 the
        // prefix before the pointer is still the nearest one below the
        // boundary (>= p[qhi]); before qlo the first end is past p[q].
        const uint32_t qlo = ps + (uint32_t)lo, qhi = ps + (uint32_t)Y;
        const uint32_t upb = (uint32_t)pb;
        uint32_t g[HIST_FAST_MAX];
        bool bad = false;
#pragma unroll
        for (int i = 0; i < KT; ++i) {  // (boundaries below k0: every end past them -- c[8] at the flush)
            const uint32_t t = ht.t[i], q = ht.q[i];
            if (q <= qhi && ht.v[i] - upb < t + (uint32_t)CUT_EPS_FX) bad = true;
            if (q > qlo && ht.pv[i] - upb + (uint32_t)CUT_EPS_FX > t) bad = true;
            const uint32_t sh = q - ps;  // q >= ps (p[q] > pb + T_k >= p[ps - 1] + 3)
            g[i] = sh >= 64u ? 0u : (uint32_t)__popcll(em >> sh);
        }
        if (bad) { r.exact = false; return r; }
#pragma unroll
        for (int i = 0; i < KT; ++i) ht.c[i] += g[i];
        ht.c[HIST_FAST_MAX] += n;
      }
    } else if (HIST && n) {
        // the buckets of the first and last end (exact ones: none within ~0.006 Da of a boundary)
        const double ml = dp.m0 + (double)D((uint32_t)lo) / CUT_SCALE, my = dp.m0 + (double)D((uint32_t)Y) / CUT_SCALE;
        const int b0 = java_d2i(ml) / dp.br, b1 = java_d2i(my) / dp.br;
        auto tb = [&](int k) { return cut_threshold((double)(k * dp.br), dp.m0); };  // boundary k x BR
        if (cut_cmp(D((uint32_t)lo), tb(b0)) <= 0 || cut_cmp(D((uint32_t)lo), tb(b0 + 1)) >= 0 ||
            cut_cmp(D((uint32_t)Y), tb(b1)) <= 0 || cut_cmp(D((uint32_t)Y), tb(b1 + 1)) >= 0) {
            r.exact = false;
            return r;
        }
        if (b1 - b0 > 7) { r.exact = false; return r; }
        uint32_t at[7];  // first position of bucket b0 + 1 + i
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            at[i] = (uint32_t)Y + 1u;
            if (i < b1 - b0) {
                const int64_t t = tb(b0 + 1 + i);
                const uint32_t a = first_above(D, (uint32_t)lo + 1u, (uint32_t)Y, t);  // m(lo) < B <= m(Y)
                if (cut_cmp(D(a), t) <= 0 || cut_cmp(D(a - 1), t) >= 0) { r.exact = false; return r; }
                at[i] = a;
            }
        }
        uint32_t from = (uint32_t)lo;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            if (i < b1 - b0) {
                if (at[i] > from) {
                    const uint32_t c = (uint32_t)__popcll(em & bit_range(from, at[i] - 1u));
                    if (c) atomicAdd(&hist[min(b0 + i, dp.nb)], c);
                }
                from = max(from, at[i]);
            }
        }
        if (from <= (uint32_t)Y) {
            const uint32_t c = (uint32_t)__popcll(em & bit_range(from, (uint32_t)Y));
            if (c) atomicAdd(&hist[min(b1, dp.nb)], c);
        }
    }
    r.kept = n - nd;
    r.dropped = nd;
    return r;
}

// Build the fixed-point prefix table from the staged window (all threads;
// ends with a barrier): fp64 sums per thread, a block scan, then each
// position's prefix rounded to 2^-9 Da
__device__ void build_cut_tables(const DigestSmem& sm, CutSmem& cs, uint32_t nbytes, double* s_dtmp) {
    constexpr uint32_t E = (WIN + DIGEST_THREADS - 1) / DIGEST_THREADS;
    const uint32_t lo = threadIdx.x * E;
    double msum = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < E; ++k) {
        const uint32_t i = lo + k;
        if (i < nbytes) msum += sm.mass[sm.win[i] & 0xFFu];
    }
    double dtot;
    double mrun = block_excl_scan<DIGEST_THREADS, double>(msum, s_dtmp, dtot);
#pragma unroll
    for (uint32_t k = 0; k < E; ++k) {
        const uint32_t i = lo + k;
        if (i < nbytes) {
            mrun += sm.mass[sm.win[i] & 0xFFu];
            cs.p(i) = (uint32_t)__double2ull_rn(mrun * CUT_SCALE);
        }
    }
    // the slack words past the window read as "above every threshold" (the
    // tracked bucket boundaries load p[q + 1], p[q + 2] unclamped)
    if (threadIdx.x < 4) cs.p(nbytes + threadIdx.x) = 0xFFFFFFFFu;
    __syncthreads();
}

template <bool HIST, bool FAST = false, int KT = 0>
__global__ void __launch_bounds__(DIGEST_THREADS) __attribute__((amdgpu_waves_per_eu(HIST ? 4 : 1, 8)))
k_digest_count_cuts(DevParams dp, const double* __restrict__ d_mass_tab, const uint8_t* __restrict__ d_flags,
                    const uint8_t* __restrict__ d_res, const uint32_t* __restrict__ d_poff, uint32_t n_prot,
                    uint32_t n_res, const uint32_t* __restrict__ d_tile_pf, uint32_t* __restrict__ d_blk,
                    uint32_t* __restrict__ d_thr, Counters* __restrict__ d_ctr,
                    unsigned long long* __restrict__ d_hist) {
    __shared__ DigestSmem sm;
    __shared__ CutSmem cs;
    __shared__ double s_dtmp[DIGEST_THREADS / 64 + 1];
    __shared__ uint32_t s_hist[HIST ? HIST_MAX_BUCKETS + 1 : 1];
    if (HIST)  // (digest_prepare's barriers come before the first count)
        for (uint32_t b = threadIdx.x; b <= (uint32_t)dp.nb; b += DIGEST_THREADS) s_hist[b] = 0;
    HistTrack ht;
    const CutLimits cl = cut_limits(dp);
    constexpr bool fast = HIST && FAST;  // (count_fast_ok on the host)
    ht.k0 = ht.k1 = 0;
#pragma unroll
    for (int k = 0; k < HIST_FAST_MAX; ++k) {
        ht.q[k] = ht.v[k] = ht.pv[k] = 0;
        // an exact start's kept ends lie at least CUT_EPS inside [minMH, maxMH]
        // in prefix units (count_by_masks' limit checks), so a boundary at or
        // below minMH is surely passed by all of them, one at or above maxMH
        // by none (SQLiteMult: a 1000-Da edge equal to maxMH, 6000 Da)
        if (k < dp.nb && cl.t_b[k] <= cl.t_min) ht.k0 = k + 1;
        if (k < dp.nb && cl.t_b[k] < cl.t_max) ht.k1 = k + 1;
    }
#pragma unroll
    for (int k = 0; k <= HIST_FAST_MAX; ++k) ht.c[k] = 0;
    const bool kt_ok = (ht.k1 > ht.k0 ? ht.k1 - ht.k0 : 0u) == (uint32_t)KT;
#pragma unroll
    for (int i = 0; i < HIST_FAST_MAX; ++i) {  // tracked boundary i = k0 + i (KT = k1 - k0, launch_digest)
        ht.t[i] = 0;
#pragma unroll
        for (int k = 0; k < HIST_FAST_MAX; ++k)
            if ((uint32_t)k == ht.k0 + (uint32_t)i) ht.t[i] = (uint32_t)cl.t_b[k];
    }
    TileCtx tc;
    const uint32_t ncand = digest_prepare<false>(sm, tc, blockIdx.x, gridDim.x, d_mass_tab, d_flags, d_res, d_poff, n_prot, n_res,
                                                 d_tile_pf, d_ctr);
    build_cut_tables(sm, cs, tc.nbytes, s_dtmp);
    uint32_t jb, je;
    thread_share(ncand, jb, je);
    uint32_t kept = 0, dropped = 0;
    for (uint32_t j = jb; j < je; ++j) {
        // (a launch whose KT is not this kernel's k1 - k0 -- never, launch_digest derives both alike --
        // walks every start)
        CutCount r{0u, 0u, false};
        if (!fast || kt_ok) r = count_by_masks<HIST, FAST, KT>(dp, cl, sm, cs, tc.nbytes, tc.t0 + sm.cand[j] - tc.w0, s_hist, ht);
        if (!r.exact) {
            const WalkOut w = walk_candidate<false, false, false, HIST>(dp, sm, tc, d_res, d_poff, j, nullptr, nullptr,
                                                                        s_hist);
            r.kept = w.kept;
            r.dropped = w.dropped;
        }
        kept += r.kept;
        dropped += r.dropped;
    }
    if (fast) {  // the register counts into the block's (wave sums: one LDS atomic per wave and bucket)
        // bucket k holds the ends past boundary k-1 and not past boundary k
        uint32_t above = ht.c[HIST_FAST_MAX];  // every end is past "boundary -1"
#pragma unroll
        for (int k = 0; k <= HIST_FAST_MAX; ++k) {
            uint32_t past = (uint32_t)k < ht.k0 ? ht.c[HIST_FAST_MAX] : 0u;  // below k0: every end; from k1: none
#pragma unroll
            for (int i = 0; i < KT; ++i)
                if ((uint32_t)k == ht.k0 + (uint32_t)i) past = ht.c[i];
            if (k >= dp.nb) past = 0u;
            const uint32_t v = k <= dp.nb ? wave_sum(above - past) : 0u;
            if (k <= dp.nb && lane_id() == 0 && v) atomicAdd(&s_hist[k], v);
            if (k < dp.nb) above = past;
        }
    }
    publish_counts(sm, kept, dropped, d_blk, d_thr, d_ctr);
    if (HIST) hist_flush(dp, s_hist, d_hist);
}

// ---------------------------------------------------------------------------
// Fused COUNT + EMIT (one staging of the window): count the tile's kept
// records, publish the tile total, find the tile's output offset by a
// decoupled look-back over earlier tiles (tiles numbered by an atomic ticket
// in dispatch order, so every predecessor is running or done), then walk again
// and emit.  Status word per tile: epoch (16 b) | state (2 b) | value (46 b),
// state 1 = tile total, 2 = inclusive prefix; agent-scope atomics.
// ---------------------------------------------------------------------------
constexpr unsigned long long ST_AGG = 1ull, ST_PREFIX = 2ull;

__device__ __forceinline__ unsigned long long st_pack(uint32_t epoch, unsigned long long state,
                                                      unsigned long long v) {
    return ((unsigned long long)epoch << 48) | (state << 46) | v;
}

// Thread 0 of tile `tile`: publish the tile's total (the first tile its
// inclusive prefix right away).
__device__ __forceinline__ void tile_publish(unsigned long long* __restrict__ status, uint32_t tile, uint32_t epoch,
                                             unsigned long long total) {
    __hip_atomic_store(&status[tile], st_pack(epoch, tile == 0 ? ST_PREFIX : ST_AGG, total), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// Wave 0 of a tile that published its total: look back 64 tiles at a time
// for the exclusive prefix (returned to every lane), publish the inclusive one.
// (Four status words per lane per round trip measured slower: the pollers'
// traffic, not the hops, is what the wait costs.)
__device__ unsigned long long tile_lookback_wait(unsigned long long* __restrict__ status, uint32_t tile,
                                                 uint32_t epoch, unsigned long long total) {
    unsigned long long excl = 0;
    int64_t t = (int64_t)tile - 1;
    const uint32_t lane = lane_id();
    while (t >= 0) {
        const int64_t q = t - (int64_t)lane;
        unsigned long long v = 0;
        bool ready = true;
        if (q >= 0) {
            v = __hip_atomic_load(&status[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ready = (uint32_t)(v >> 48) == epoch && ((v >> 46) & 3ull) != 0;
        }
        const uint64_t pref = __ballot(q >= 0 && ready && ((v >> 46) & 3ull) == ST_PREFIX);
        const uint64_t notready = __ballot(!ready);
        // lanes up to (and including) the nearest prefix, all ready -> sum them
        const uint32_t upto = pref ? (uint32_t)__ffsll((long long)pref) - 1 : 64u;  // nearest prefix lane
        const uint64_t need = upto >= 63 ? ~0ull : ((2ull << upto) - 1);
        if (notready & need) continue;  // a predecessor has not published yet: poll again
        const unsigned long long val = (lane <= upto && q >= 0) ? (v & ((1ull << 46) - 1)) : 0ull;
        excl += wave_sum(val);
        if (pref) break;
        t -= 64;
    }
    if (threadIdx.x == 0 && tile != 0)
        __hip_atomic_store(&status[tile], st_pack(epoch, ST_PREFIX, excl + total), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    return excl;
}

// Wave 0 of tile `tile`: publish the tile's total, then the look-back.
__device__ unsigned long long tile_lookback(unsigned long long* __restrict__ status, uint32_t tile, uint32_t epoch,
                                            unsigned long long total) {
    if (threadIdx.x == 0) tile_publish(status, tile, epoch, total);
    return tile_lookback_wait(status, tile, epoch, total);
}

template <bool SEMI, bool MAND, bool FILT = false>
__global__ void __launch_bounds__(DIGEST_THREADS)
k_digest_fused(DevParams dp, const double* __restrict__ d_mass_tab, const uint8_t* __restrict__ d_flags,
               const uint8_t* __restrict__ d_res, const uint32_t* __restrict__ d_poff, uint32_t n_prot,
               uint32_t n_res, const uint32_t* __restrict__ d_tile_pf, unsigned long long* __restrict__ status,
               uint32_t epoch, Rec* __restrict__ d_out, uint32_t cap, Counters* __restrict__ d_ctr) {
    __shared__ DigestSmem sm;
    __shared__ uint32_t s_tile;
    __shared__ unsigned long long s_base;
    if (threadIdx.x == 0) s_tile = atomicAdd(&d_ctr->tile_ticket, 1u);
    __syncthreads();
    const uint32_t tile = s_tile;
    TileCtx tc;
    const uint32_t ncand = digest_prepare<SEMI>(sm, tc, tile, gridDim.x, d_mass_tab, d_flags, d_res, d_poff, n_prot, n_res,
                                                d_tile_pf, d_ctr);
    uint32_t jb, je;
    thread_share(ncand, jb, je);
    // count (exact walk: the cut-stepping tables would cost this kernel its
    // occupancy, and its emit walk is issue-bound)
    uint32_t kept = 0, dropped = 0;
    for (uint32_t j = jb; j < je; ++j) {
        const WalkOut w = walk_candidate<false, SEMI, MAND, false, FILT>(dp, sm, tc, d_res, d_poff, j, nullptr, nullptr);
        kept += w.kept;
        dropped += w.dropped;
    }
    uint32_t total;
    const uint32_t mine = block_excl_scan<DIGEST_THREADS, uint32_t>(kept, sm.tmp, total);
    const uint32_t td = block_sum<DIGEST_THREADS, uint32_t>(dropped, sm.tmp);
    if (threadIdx.x < 64) {
        const unsigned long long excl = tile_lookback(status, tile, epoch, total);
        if (threadIdx.x == 0) {
            if (td) atomicAdd(&d_ctr->n_dropped, (unsigned long long)td);
            if (tile == gridDim.x - 1) d_ctr->n_kept = excl + total;
            s_base = excl;
        }
    }
    __syncthreads();
    tc.w = rec_width(d_ctr->max_plen);
    if (tile == 0 && threadIdx.x == 0 && !rec_layout_ok(tc.w, n_prot)) atomicOr(&d_ctr->err, ERR_LAYOUT);
    const unsigned long long base = s_base + mine;
    Rec* out = d_out + base;
    const Rec* out_end = d_out + cap;
    for (uint32_t j = jb; j < je; ++j)
        out += walk_candidate<true, SEMI, MAND, false, FILT>(dp, sm, tc, d_res, d_poff, j, out, out_end).kept;
}

hipError_t launch_digest_fused(const DevParams& dp, const double* d_mass_tab, const uint8_t* d_flags,
                               const uint8_t* d_res, const uint32_t* d_poff, uint32_t n_prot, uint32_t n_res,
                               const uint32_t* d_tile_pf, unsigned long long* d_status, uint32_t epoch,
                               Rec* d_out, uint32_t cap, Counters* d_ctr, hipStream_t s) {
    const uint32_t nblk = (n_res + DIGEST_TILE - 1) / DIGEST_TILE;
    if (nblk == 0) return hipSuccess;
#define DBI_FUSED(SEMI, MAND)                                                                                 \
    do {                                                                                                      \
        if (dp.pf_kind)                                                                                       \
            DBI_LAUNCH((k_digest_fused<SEMI, MAND, true>), dim3(nblk), dim3(DIGEST_THREADS), 0, s, dp,        \
                       d_mass_tab, d_flags, d_res, d_poff, n_prot, n_res, d_tile_pf, d_status, epoch, d_out,  \
                       cap, d_ctr);                                                                           \
        else                                                                                                  \
            DBI_LAUNCH((k_digest_fused<SEMI, MAND>), dim3(nblk), dim3(DIGEST_THREADS), 0, s, dp, d_mass_tab,  \
                       d_flags, d_res, d_poff, n_prot, n_res, d_tile_pf, d_status, epoch, d_out, cap, d_ctr); \
    } while (0)
    if (dp.semi) {
        if (dp.mand_mode) DBI_FUSED(true, true); else DBI_FUSED(true, false);
    } else {
        if (dp.mand_mode) DBI_FUSED(false, true); else DBI_FUSED(false, false);
    }
#undef DBI_FUSED
    return hipGetLastError();
}

// Length-balanced walk order.  A full-enzyme walk from candidate j ends near
// the B-th next cleavage site, so cand[j+B] - cand[j] estimates its length; a
// counting sort of the candidates by that estimate (in place, through
// registers) gives each wave's lanes walks of about the same length, instead
// of every wave waiting for its longest one.  Any order is valid: each
// candidate's records go to the slots its thread reserved for it.  Tiles of
// more than BAL_MAX candidates keep their order.  s_cnt: BAL_BUCKETS words.
constexpr uint32_t BAL_ITEMS = 4;
constexpr uint32_t BAL_MAX = BAL_ITEMS * DIGEST_THREADS;
constexpr uint32_t BAL_BUCKETS = 128;

__device__ void balance_candidates(uint16_t* cand, uint32_t* s_cnt, uint32_t ncand, uint32_t B, uint32_t tile_len) {
    if (ncand > BAL_MAX || ncand < 2) return;  // block-uniform
    for (uint32_t b = threadIdx.x; b < BAL_BUCKETS; b += DIGEST_THREADS) s_cnt[b] = 0;
    __syncthreads();
    uint32_t cv[BAL_ITEMS], key[BAL_ITEMS], rk[BAL_ITEMS];
#pragma unroll
    for (uint32_t k = 0; k < BAL_ITEMS; ++k) {
        const uint32_t j = threadIdx.x + k * DIGEST_THREADS;
        if (j < ncand) {
            cv[k] = cand[j];
            const uint32_t nxt = j + B < ncand ? cand[j + B] : tile_len + (uint32_t)DIGEST_HALO;
            key[k] = min(nxt - cv[k], BAL_BUCKETS - 1);
            rk[k] = atomicAdd(&s_cnt[key[k]], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {  // exclusive scan of the bucket counts, one wave
        constexpr uint32_t PER = BAL_BUCKETS / 64;
        uint32_t v[PER], loc = 0;
#pragma unroll
        for (uint32_t q = 0; q < PER; ++q) {
            v[q] = s_cnt[threadIdx.x * PER + q];
            loc += v[q];
        }
        uint32_t run = wave_incl_scan(loc) - loc;
#pragma unroll
        for (uint32_t q = 0; q < PER; ++q) {
            s_cnt[threadIdx.x * PER + q] = run;
            run += v[q];
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < BAL_ITEMS; ++k) {
        const uint32_t j = threadIdx.x + k * DIGEST_THREADS;
        if (j < ncand) cand[s_cnt[key[k]] + rk[k]] = (uint16_t)cv[k];
    }
    __syncthreads();
}

// Offset of the k-th set bit (k >= 1) of the 128-bit map (lo, hi), 128 if
// it has fewer than k.
__device__ __forceinline__ uint32_t kth_bit_128(uint64_t lo, uint64_t hi, uint32_t k) {
    const uint32_t nlo = (uint32_t)__popcll(lo);
    uint64_t x = lo;
    uint32_t base = 0;
    if (nlo < k) {
        k -= nlo;
        x = hi;
        base = 64;
        if ((uint32_t)__popcll(hi) < k) return 128u;
    }
    for (uint32_t q = 1; q < k; ++q) x &= x - 1;  // drop the first k-1
    return base + (uint32_t)__ffsll((long long)x) - 1;
}

// first set bit of the 128-bit map (lo, hi), 128 if none
__device__ __forceinline__ uint32_t first_bit_128(uint64_t lo, uint64_t hi) {
    return lo ? (uint32_t)__ffsll((long long)lo) - 1u : hi ? 64u + (uint32_t)__ffsll((long long)hi) - 1u : 128u;
}

// bits [0, x) of a 64-bit word, x <= 64
__device__ __forceinline__ uint64_t low_bits(uint32_t x) { return x >= 64 ? ~0ull : ((1ull << x) - 1ull); }

template <uint32_t R>
__device__ void part_tile(const PartOut& po, const Rec* __restrict__ src, uint32_t n, uint32_t* s_cnt,
                          uint32_t* s_run, uint32_t* s_tmp, uint4* stage, uint16_t* sdig, Counters* __restrict__ ctr);

// ---------------------------------------------------------------------------
// Bounded semi-specific digest (no mandatory residues, no windows; warm
// builds): one walk per start instead of the fused kernel's count walk +
// look-back + emit walk.  Every start is a candidate (checkCleavage = N_ok ||
// C_ok, DBIndexer.java:318), and a start's records are ends e, ascending, with
//   s + MIN_PEP_LENGTH - 1 <= e < stop,  stop = the (maxMC+2)-th cleave residue
//   from s (mc > maxMC from there on: every later cut breaks, :322-324, and no
//   end after it emits) or the next protein's first residue (:284),
// at every such position when N_ok(s) holds, else at the cuts only -- minus
// the mass filters (minMH / maxMH / the bucket drop), which only remove
// records.  So the bit maps bound a start's records before its walk; a start
// whose stop lies past the 128-position horizon is counted by its exact walk
// instead.  Tiles reserve the bound by one atomic add (any tile order: the
// chunk sort restores first appearance, ck_fix_runs), each walk writes its
// records into its slots, and the unused slots get REC_SENTINEL, which the
// first radix pass drops -- as in k_digest_bounded.
// ---------------------------------------------------------------------------
// PART: the tile's records partitioned afterwards into the regions of their
// fine bins' low digit (part_tile, PartOut::lsd: the radix tail's first pass,
// fused; the slots are scratch).
template <bool DROP, bool PART = false>
__global__ void __launch_bounds__(DIGEST_THREADS)
k_digest_semi_bounded(DevParams dp, const double* __restrict__ d_mass_tab, const uint8_t* __restrict__ d_flags,
                      const uint8_t* __restrict__ d_res, const uint32_t* __restrict__ d_poff, uint32_t n_prot,
                      uint32_t n_res, const uint32_t* __restrict__ d_tile_pf, Rec* __restrict__ d_out, uint64_t cap,
                      Counters* __restrict__ d_ctr, PartOut po) {
    __shared__ DigestSmem sm;
    __shared__ unsigned long long s_base;
    TileCtx tc;
    const uint32_t ncand = digest_prepare<true>(sm, tc, blockIdx.x, gridDim.x, d_mass_tab, d_flags, d_res, d_poff,
                                                n_prot, n_res, d_tile_pf, d_ctr);
    uint32_t jb, je;
    thread_share(ncand, jb, je);
    const uint32_t kcl = (uint32_t)dp.max_missed + 2u;
    const uint32_t a = dp.min_len > 0 ? (uint32_t)dp.min_len - 1u : 0u;  // first end, relative (:331)
    const uint32_t known = tc.w_end == n_res ? tc.nbytes - 1u : tc.nbytes - 2u;  // last window position with its cut bit
    // slot bounds (an open start: its exact count, the walk run twice)
    uint32_t lim = 0;
    for (uint32_t j = jb; j < je; ++j) {
        const uint32_t i = sm.cand[j];
        const uint32_t p = tc.t0 - tc.w0 + i;  // window position of the start
        const uint64_t cl0 = bits_from(sm.clvm, p), cl1 = bits_from(sm.clvm, p + 64);
        const uint64_t st0 = bits_from(sm.stm, p) & ~1ull, st1 = bits_from(sm.stm, p + 64);
        const uint32_t stop = min(kth_bit_128(cl0, cl1, kcl), first_bit_128(st0, st1));
        const uint32_t horizon = min(127u, known - p);
        if (stop >= 128u || stop > horizon + 1u) {  // (128: no stop within the horizon)
            lim += walk_candidate<false, true, false>(dp, sm, tc, d_res, d_poff, j, nullptr, nullptr).kept;
        } else if (stop > a) {
            if (n_ok_at(sm, tc, i)) {
                lim += stop - a;
            } else {
                const uint64_t c0 = bits_from(sm.cutm, p), c1 = bits_from(sm.cutm, p + 64);
                lim += (uint32_t)__popcll(c0 & low_bits(min(stop, 64u)) & ~low_bits(min(a, 64u))) +
                       (uint32_t)__popcll(c1 & low_bits(stop > 64u ? stop - 64u : 0u) & ~low_bits(a > 64u ? a - 64u : 0u));
            }
        }
    }
    uint32_t tile_slots;
    const uint32_t excl_t = block_excl_scan<DIGEST_THREADS, uint32_t>(lim, sm.tmp, tile_slots);
    if (threadIdx.x == 0) s_base = atomicAdd(&d_ctr->n_slots, (unsigned long long)tile_slots);
    __syncthreads();
    const unsigned long long base = s_base;
    if (base + tile_slots > cap) return;  // too small: the caller grows it and runs again
    tc.w = rec_width(d_ctr->max_plen);
    if (blockIdx.x == 0 && threadIdx.x == 0 && !rec_layout_ok(tc.w, n_prot)) atomicOr(&d_ctr->err, ERR_LAYOUT);
    Rec* __restrict__ o = d_out + base + excl_t;
    uint32_t kept = 0, dropped = 0;
    for (uint32_t j = jb; j < je; ++j) {
        const WalkOut w = walk_candidate<true, true, false>(dp, sm, tc, d_res, d_poff, j, o + kept, o + lim);
        kept += w.kept;
        dropped += w.dropped;
    }
    if (kept > lim) atomicOr(&d_ctr->err, ERR_SLOTS);  // the bound is an upper bound: never
    const Rec sent{REC_SENTINEL, REC_SENTINEL};
    for (uint32_t k = kept; k < lim; ++k) o[k] = sent;
    const uint32_t tk = block_sum<DIGEST_THREADS, uint32_t>(kept, sm.tmp);
    const uint32_t td = DROP ? block_sum<DIGEST_THREADS, uint32_t>(dropped, sm.tmp) : 0u;
    if (threadIdx.x == 0) {
        if (tk) atomicAdd(&d_ctr->n_kept, (unsigned long long)tk);
        if (td) atomicAdd(&d_ctr->n_dropped, (unsigned long long)td);
    }
    if constexpr (PART) {  // the walks' LDS is dead: the counters in the mass table, the stage over the rest
        constexpr size_t b0 = offsetof(DigestSmem, nokm), b1 = offsetof(DigestSmem, tmp);
        constexpr uint32_t R = (uint32_t)((b1 - b0) / 18 / 64 * 64);  // 16 B + 2 B per staged record
        static_assert(b0 % 16 == 0 && R >= 512 && sizeof(sm.mass) >= 512 * sizeof(uint32_t), "partition stage");
        uint8_t* st = reinterpret_cast<uint8_t*>(&sm) + b0;
        uint32_t* p_cnt = reinterpret_cast<uint32_t*>(sm.mass);
        part_tile<R>(po, d_out + base, tile_slots, p_cnt, p_cnt + 256, sm.tmp, reinterpret_cast<uint4*>(st),
                     reinterpret_cast<uint16_t*>(st + 16 * R), d_ctr);
    }
}

hipError_t launch_digest_semi_bounded(const DevParams& dp, const double* d_mass_tab, const uint8_t* d_flags,
                                      const uint8_t* d_res, const uint32_t* d_poff, uint32_t n_prot, uint32_t n_res,
                                      const uint32_t* d_tile_pf, Rec* d_out, uint64_t cap, Counters* d_ctr,
                                      hipStream_t s, const PartOut* part) {
    const uint32_t nblk = (n_res + DIGEST_TILE - 1) / DIGEST_TILE;
    if (nblk == 0) return hipSuccess;
    if (!dp.semi || dp.mand_mode || dp.filter) return hipErrorInvalidValue;
    PartOut po{};
    if (part) {
        if (!part->lsd || part->b1 < 1 || part->b1 > 8 || part->dm.b2 < 1 || part->dm.b2 > RADIX_BITS || part->cap % 64)
            return hipErrorInvalidValue;
        po = *part;
    }
#define DBI_DIGEST_S(DROP, PART)                                                                                     \
    DBI_LAUNCH((k_digest_semi_bounded<DROP, PART>), dim3(nblk), dim3(DIGEST_THREADS), 0, s, dp, d_mass_tab, d_flags, \
               d_res, d_poff, n_prot, n_res, d_tile_pf, d_out, cap, d_ctr, po)
    const bool drop = dp.drop_mass <= dp.max_mh;
    if (part) {
        if (drop) DBI_DIGEST_S(true, true);
        else DBI_DIGEST_S(false, true);
    } else {
        if (drop) DBI_DIGEST_S(true, false);
        else DBI_DIGEST_S(false, false);
    }
#undef DBI_DIGEST_S
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Bounded digest (full enzyme, no mandatory residues, <= 2 missed cleavages;
// warm builds): one walk per cleavage-site start, into slots reserved by a
// decoupled look-back.  A full-enzyme walk emits only at cuts, and every
// limit is monotone along it (the mass only grows, intMisCleavageCount only
// grows), so the records of start s are the cuts e, in ascending order, with
//   s + MIN_PEP_LENGTH - 1 <= e < stop  and  minMH <= m(e) <= maxMH,
//   stop = the (maxMC+2)-th cleave residue from s (from there on every cut
//          breaks, DBIndexer.java:322-324) or the first residue of the next
//          protein (:284 end < length), whichever comes first
// (the bucket drop, :282-288 of SQLiteMult, counts instead of keeping; the
// filterSequence of a non-mandatory store is INCLUDE for every such mass).
// The cut, cleave and protein-start bit maps of the staged window give those
// candidate ends (<= maxMC + 2, within a 128-position horizon) before the walk
// starts, so the residue loop is only the sequential fp64 sum (:306-308,
// -ffp-contract=off) up to the last candidate end, with the mass at each end
// parked in LDS; the records (mass filters, tag from the peptide's end bytes)
// are written after the loop.  A start whose stop lies past the horizon (no
// protein end and fewer than maxMC+2 cleave residues within 128 positions)
// and whose mass is still <= maxMH there is redone from HBM (walk_global).
// The window holds raw residue bytes (16-B LDS stores of the 16-B loads) at
// LDS position q = global index - w0 + lb, lb = 16 + the misalignment of
// d_res + w0, so every 16-B global vector lands on a 16-B LDS slot and the
// cleave / no-cut bit maps are written as plain 16-bit slices.
// ---------------------------------------------------------------------------
constexpr int LD_PRE = 16;                          // residues staged before the tile (N_ok of its first start)
constexpr int LD_HORIZON = 128;                     // positions a walk reads from LDS
constexpr int LD_HALO = LD_HORIZON + 16;            // past the tile: the horizon + the residue after it
constexpr int LD_WIN = 32 + LD_PRE + DIGEST_TILE + LD_HALO;  // + lb (16 + alignment pad)
constexpr int LD_WORDS = LD_WIN / 64 + 2;
constexpr int LD_ENDS = 4;                          // candidate ends of one start, at most (maxMC + 2)

template <uint32_t POOL>
struct LeanSmemT {
    double mass[256];
    uint32_t tmp[DIGEST_THREADS / 64 + 1];
    alignas(16) uint64_t clvm[LD_WORDS];  // bit q: cleave residue at LDS position q
    uint64_t cutm[LD_WORDS];  // bit q: checkCleavage's C side holds at q (protein ends included)
    uint64_t stm[LD_WORDS];   // bit q: a protein starts at q (one past the window included)
    uint32_t pst[PST_CAP];    // poff[pf .. pl+1] (protein of a start: binary search)
    uint16_t wpre[LD_WORDS];  // protein starts marked in stm words before word w
    alignas(16) uint8_t win[LD_WIN + 16];
    uint8_t flags[256];
    // the candidate starts (u16, tile-local, compacted, then balanced), then
    // the walks' scratch: the masses at a walk's candidate ends ([end][thread],
    // endm()), or -- a staged PART tile -- the tile's records; before the
    // walks the no-cut and N_ok maps and the balance counts (behind the list)
    alignas(16) uint8_t pool[POOL];
    __device__ __forceinline__ uint16_t* cand() { return reinterpret_cast<uint16_t*>(pool); }
    __device__ __forceinline__ const uint16_t* cand() const { return reinterpret_cast<const uint16_t*>(pool); }
    __device__ __forceinline__ double* endm() { return reinterpret_cast<double*>(pool + 2 * DIGEST_TILE); }
    __device__ __forceinline__ const double* endm() const {
        return reinterpret_cast<const double*>(pool + 2 * DIGEST_TILE);
    }
};
constexpr uint32_t LD_POOL = 2 * DIGEST_TILE + LD_ENDS * DIGEST_THREADS * 8;
using LeanSmem = LeanSmemT<LD_POOL>;
static_assert((2 * LD_WORDS * 8 + 4 * BAL_BUCKETS) <= LD_ENDS * DIGEST_THREADS * 8, "scratch inside endm");
static_assert(LD_ENDS * DIGEST_THREADS * 8 % 16 == 0, "endm layout");
// The partitioning digest (PART) keeps a tile's records in LDS while they are
// written (stage mode, below): its pool takes every byte up to 26 KiB a block
// (6 blocks per CU, the occupancy of the plain digest), so a tile of ~1 100
// records (SwissProt: 1 106 on average, 1 302 at most) fits beside the list of
// its ~460 candidate starts at 12 B a record.
constexpr uint32_t LD_LDS_PART = 26624;
constexpr uint32_t LD_HEAD = (uint32_t)sizeof(LeanSmemT<16>) - 16u;
constexpr uint32_t LD_POOL_PART = (LD_LDS_PART - LD_HEAD - 64u) & ~15u;
using LeanSmemP = LeanSmemT<LD_POOL_PART>;
static_assert(LD_POOL_PART >= LD_POOL, "the PART pool holds the plain one");

// Protein of start s: largest p in [pf, pl] with poff[p] <= s (LDS copy of
// the tile's offsets, HBM when they did not fit), and its first residue.
__device__ __forceinline__ uint32_t protein_of(const uint32_t* pst, uint32_t npst, uint32_t pf, uint32_t pl,
                                               const uint32_t* __restrict__ d_poff, uint32_t s, uint32_t& pstart) {
    if (npst) {
        uint32_t lo = 0, hi = npst - 1;  // pst[hi] = poff[pl+1] > s
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pst[mid] <= s) lo = mid; else hi = mid;
        }
        pstart = pst[lo];
        return pf + lo;
    }
    const uint32_t p = find_le(d_poff, pf, pl + 1, s);
    pstart = d_poff[p];
    return p;
}

struct LeanEnds {
    uint64_t lo, hi;   // candidate ends: bit r = LDS position p + r
    uint32_t horizon;  // last position (relative) the walk may read from LDS
    bool open;         // the walk may go on past the horizon (more ends there)
};

// known: last LDS position whose cut bit is known (the window's last one only
// at the end of the residues)
template <typename SM>
__device__ __forceinline__ LeanEnds lean_ends(const SM& sm, uint32_t p, uint32_t known, uint32_t kcl,
                                              uint32_t min_len) {
    const uint64_t cl0 = bits_from(sm.clvm, p), cl1 = bits_from(sm.clvm, p + 64);
    const uint64_t st0 = bits_from(sm.stm, p) & ~1ull, st1 = bits_from(sm.stm, p + 64);
    const uint32_t stop = min(kth_bit_128(cl0, cl1, kcl), first_bit_128(st0, st1));
    LeanEnds e;
    e.horizon = min((uint32_t)LD_HORIZON - 1u, known - p);
    // past the horizon: a stop beyond the window's known cut bits, or none
    // within LD_HORIZON positions (kth / first_bit_128 return 128) -- a walk
    // through residues light enough to stay <= maxMH over 128 positions
    e.open = stop >= (uint32_t)LD_HORIZON || stop > e.horizon + 1u;
    const uint32_t a = min_len > 0 ? min_len - 1u : 0u;  // pepSize >= MIN_PEP_LENGTH (:331)
    const uint32_t b = min(stop, e.horizon + 1u);        // ends in [a, b)
    e.lo = bits_from(sm.cutm, p) & low_bits(min(b, 64u)) & ~low_bits(min(a, 64u));
    e.hi = bits_from(sm.cutm, p + 64) & low_bits(b > 64u ? b - 64u : 0u) & ~low_bits(a > 64u ? a - 64u : 0u);
    return e;
}

// One start at LDS position p, in two halves: lean_masses runs the residue
// loop and parks the mass at each candidate end in LDS; lean_emit writes the
// records.  Between them the block may wait for its slot base (the first
// walk of every thread overlaps the tile's look-back).
struct LeanWalk {
    uint32_t pk;     // candidate end positions, one byte each, ascending (0xFF: none)
    uint32_t nreal;  // candidate ends (the horizon entry, if any, is not one)
    uint32_t j;      // masses parked
    bool overflow;   // the walk goes on past the horizon: redo it with walk_global
};

// em[k * es]: where the mass at the walk's k-th listed end is parked
template <typename SM>
__device__ __forceinline__ LeanWalk lean_masses(const DevParams& dp, const SM& sm, uint32_t p, const LeanEnds& en,
                                                double* __restrict__ em, uint32_t es) {
    LeanWalk w{~0u, 0u, 0u, false};
    double m = dp.m0;
    if (!(m <= dp.max_mh)) return w;  // while condition before the first residue (:284)
    // a walk that may leave the horizon also parks the mass at the horizon
    // (its last entry), which decides whether it is redone from HBM
    uint32_t pk = ~0u, last = 0, nreal = 0;
    {
        uint64_t lo = en.lo, hi = en.hi;
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)LD_ENDS; ++k) {
            const uint32_t b = first_bit_128(lo, hi);
            if (b < 128u) {
                pk = (pk & ~(0xFFu << (8 * k))) | (b << (8 * k));
                last = b;
                ++nreal;
            }
            if (lo) lo &= lo - 1; else hi &= hi - 1;
        }
    }
    uint32_t nlist = nreal;
    if (en.open) {  // nreal <= maxMC + 1 here: the horizon fits the list
        if (nreal == 0 || last != en.horizon) {
            pk = (pk & ~(0xFFu << (8 * nreal))) | (en.horizon << (8 * nreal));
            ++nlist;
        }
        last = en.horizon;
    }
    w.pk = pk;
    w.nreal = nreal;
    if (nlist == 0) return w;  // no candidate end
    // the residue loop, four positions per step: one dword pair of the window,
    // four mass reads in flight, then the sequential fp64 adds (:306-308); the
    // mass at each listed end goes to LDS, tested once per step (an end in
    // [q, q+4): the list is ascending and 0xFF-padded, q + 4 <= 132).
    // Positions past `last` (at most 3) only add to a mass that is no longer used.
    const uint32_t* __restrict__ w32 = reinterpret_cast<const uint32_t*>(sm.win);
    uint32_t ne = pk & 0xFFu, rest = pk, j = 0;
    for (uint32_t q = 0; q <= last; q += 4) {
        const uint32_t a = p + q;
        const uint32_t r4 = __builtin_amdgcn_alignbyte(w32[(a >> 2) + 1], w32[a >> 2], a & 3u);
        const double x0 = sm.mass[r4 & 0xFFu], x1 = sm.mass[(r4 >> 8) & 0xFFu];
        const double x2 = sm.mass[(r4 >> 16) & 0xFFu], x3 = sm.mass[r4 >> 24];
        const double m0 = m + x0, m1 = m0 + x1, m2 = m1 + x2, m3 = m2 + x3;
        while (ne < q + 4u) {
            const uint32_t d = ne - q;
            em[j * es] = d == 0u ? m0 : d == 1u ? m1 : d == 2u ? m2 : m3;
            ++j;
            rest = (rest >> 8) | 0xFF000000u;  // 0xFF past the list
            ne = rest & 0xFFu;
        }
        m = m3;
        if (m > dp.max_mh) break;  // no later end passes maxMH (:326-329, :284)
    }
    w.j = j;
    // still <= maxMH at the horizon: the walk goes on past it
    w.overflow = en.open && j == nlist && em[(nlist - 1) * es] <= dp.max_mh;
    return w;
}

// The first radix pass's histogram, counted where the records are written
// (warm bounded builds): record slot s is in radix chunk s / RADIX_CHUNK_D;
// the tile's first K chunks count in LDS (flushed by the last wave with one
// global atomic per nonzero entry), later ones -- tiles above K-1 chunks of
// slots, rare -- straight into the global histogram (zeroed before the digest).
constexpr uint32_t RADIX_CHUNK_D = RADIX_THREADS * RADIX_ITEMS;
constexpr uint32_t H1_LDS = 384;  // LDS counters: K = H1_LDS >> bits chunks of 2^bits digits
struct Hist1 {
    uint32_t* __restrict__ g;  // hist[d * G + chunk], nullptr: not counted here
    BinMap bm;
    uint32_t bits, G;
};

__device__ __forceinline__ void hist1_count(const Hist1& h1, uint32_t* s_h1, uint32_t c0, double m, uint32_t slot) {
    const uint32_t d = bin_of(m, h1.bm) & ((1u << h1.bits) - 1u);
    const uint32_t c = slot / RADIX_CHUNK_D;
    const uint32_t k = c - c0;
    if (k < (H1_LDS >> h1.bits)) atomicAdd(&s_h1[(k << h1.bits) + d], 1u);
    else atomicAdd(&h1.g[(size_t)d * h1.G + c], 1u);
}

// The records of a lean walk (not overflowed) into out[0, kept); slot: the
// global slot of out[0] (first-pass histogram, when h1.g is set).
template <bool DROP, bool H1, typename SM>
__device__ __forceinline__ WalkOut lean_emit(const DevParams& dp, const SM& sm, uint32_t p, const LeanWalk& w,
                                             const double* __restrict__ em, uint64_t loc, Rec* __restrict__ out,
                                             const Hist1& h1, uint32_t* s_h1, uint32_t c0, uint32_t slot) {
    WalkOut r{0u, 0u, false};
    const uint32_t* __restrict__ w32 = reinterpret_cast<const uint32_t*>(sm.win);
    const uint32_t head = __builtin_amdgcn_alignbyte(w32[(p >> 2) + 1], w32[p >> 2], p & 3u);
    uint32_t kept = 0, dropped = 0;
    const uint32_t nk = min(w.j, w.nreal);
    for (uint32_t k = 0; k < nk; ++k) {
        const double mk = em[k * DIGEST_THREADS];  // (lean_masses' es)
        if (!(mk <= dp.max_mh)) break;
        if (!(mk >= dp.min_mh)) continue;  // :331
        if (DROP && mk >= dp.drop_mass) {  // bucket > NUM_BUCKETS-1
            ++dropped;
            continue;
        }
        const uint32_t e = (w.pk >> (8 * k)) & 0xFFu;
        const uint32_t q = p + e - 3u;  // p >= 16
        const uint32_t tail = __builtin_bswap32(__builtin_amdgcn_alignbyte(w32[(q >> 2) + 1], w32[q >> 2], q & 3u));
        const uint32_t tag = peptide_tag(head, tail, e + 1u);
        Rec rec;
        rec.q0 = rec_q0(mk, tag);
        rec.q1 = rec_q1(tag, loc, e + 1u);
        if constexpr (H1) hist1_count(h1, s_h1, c0, mk, slot + kept);
        out[kept++] = rec;
    }
    r.kept = kept;
    r.dropped = dropped;
    return r;
}

// A staged PART tile (k_digest_bounded, stage mode): a record waits in LDS
// as 12 B -- its mass and (candidate index << STAGE_LEN_BITS | length) --
// until the tile is partitioned; the tag, protein and offset are rebuilt
// from the window there.  The walk's end masses are parked in the record
// slots themselves (em, stride 1), and lean_stage compacts the kept ones to
// the front of them.
constexpr uint32_t STAGE_LEN_BITS = 20;  // lengths < 2^20 (max_plen checked per tile)
constexpr uint32_t STAGE_NONE = ~0u;     // an unused slot of the tile's bound

template <bool DROP>
__device__ __forceinline__ WalkOut lean_stage(const DevParams& dp, const LeanWalk& w, double* __restrict__ em,
                                              uint32_t* __restrict__ ei, uint32_t j) {
    WalkOut r{0u, 0u, false};
    uint32_t kept = 0, dropped = 0;
    const uint32_t nk = min(w.j, w.nreal);
    for (uint32_t k = 0; k < nk; ++k) {
        const double mk = em[k];
        if (!(mk <= dp.max_mh)) break;
        if (!(mk >= dp.min_mh)) continue;  // :331
        if (DROP && mk >= dp.drop_mass) {  // bucket > NUM_BUCKETS-1
            ++dropped;
            continue;
        }
        em[kept] = mk;
        ei[kept++] = j << STAGE_LEN_BITS | (((w.pk >> (8 * k)) & 0xFFu) + 1u);
    }
    r.kept = kept;
    r.dropped = dropped;
    return r;
}

struct StageSink {  // walk_global's records of a staged tile
    double* __restrict__ em;
    uint32_t* __restrict__ ei;
    uint32_t j, room;
    __device__ __forceinline__ void operator()(uint32_t k, double m, uint32_t, uint32_t len) const {
        if (k < room) {
            em[k] = m;
            ei[k] = j << STAGE_LEN_BITS | len;
        }
    }
};

// ---- depth bins: the digest's partition ------------------------------------
// the bin of sub-bin sb from its map word e = dm.map[sb >> 6]
__device__ __forceinline__ uint32_t depth_bin_of(const uint4& e, uint32_t sb, const DepthMap& dm) {
    const uint64_t mask = (uint64_t)e.y << 32 | e.x;
    const uint32_t b = e.z + (uint32_t)__popcll(mask & (~0ull >> (63u - (sb & 63u))));
    return min(b, dm.last);  // (a map whose starts outnumber the bins: the top ones share the last)
}
__device__ __forceinline__ uint32_t depth_bin(double m, const DepthMap& dm) {
    const uint32_t sb = bin_of(m, dm.sub);
    return depth_bin_of(dm.map[sb >> 6], sb, dm);
}

// the XCD this wave runs on (HW_REG_XCC_ID, bits 3:0; MI355X_MICROARCH.md: blockIdx % 8 only says
// which blocks share one)
__device__ __forceinline__ uint32_t xcc_id() {
    return (uint32_t)__builtin_amdgcn_s_getreg(20 | (0 << 6) | ((4 - 1) << 11)) & (DEPTH_XCDS - 1u);
}

// The tile's records (slots [0, n) of src, just written by this block:
// L2-resident) into the regions of their bins' high digits, PART_R slots a
// round: each record's rank inside its digit from an LDS counter, the digit
// counts scanned, one L2 atomic per digit present reserves the tile's run in
// region (digit, this XCD) -- the runs of one XCD's tiles are neighbours in
// its regions, so its L2 merges their partial lines -- the records staged in
// LDS in digit order (the walks' LDS is dead) and written as digit runs by
// consecutive lanes, with their bins' low digits (pass 2 counts those bytes).
// A region that would overflow takes nothing and flags the build (ERR_PART:
// redone by the radix tail).  The records never go through a full radix pass
// of their own: this is the first pass, fused.
// s_cnt / s_run: 256 words each; stage: PART_R x 16 B, then PART_R x 2 B.
// A tile of more than R records (semi-specific: ~20 k) takes several rounds.
// Measured without gain there: counting a tile's digits first and reserving
// each digit's run once, so that the rounds need no global atomic (semi-tryptic
// digest 24.1 -> 25.8 ms), and loading the next round's records while one is
// written (24.8 ms): the partition moves its bytes (the slots read back, the
// regions written) at about the copy rate.
// One round: rv[k] = record k * DIGEST_THREADS + tid of the round (nr of
// them; REC_SENTINEL q0: none), s_cnt zeroed behind a barrier the caller put
// after its last read of the stage.
template <uint32_t KI>
__device__ __forceinline__ void part_place(const PartOut& po, const uint4 (&rv)[KI], uint32_t nr, uint32_t* s_cnt,
                                           uint32_t* s_run, uint32_t* s_tmp, uint4* stage, uint16_t* sdig,
                                           Counters* __restrict__ ctr, unsigned long long* clk = nullptr) {
#ifdef DBI_DIGEST_CLOCK
#define PCLK(k) do { if (clk && threadIdx.x == 0) clk[k] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define PCLK(k) do { } while (0)
#endif
    const uint32_t tid = threadIdx.x, xcd = xcc_id(), D1 = 1u << po.b1;
    const uint32_t b2 = po.dm.b2, m2 = (1u << b2) - 1u;
    // the region digit of a bin (depth: its high b1 bits; lsd: its low b1 bits) and its pass-2 digit
    auto d1_of = [&](uint32_t b) { return po.lsd ? b & (D1 - 1u) : b >> b2; };
    auto d2_of = [&](uint32_t b) { return po.lsd ? (b >> po.b1) & m2 : b & m2; };
    uint4* __restrict__ out4 = reinterpret_cast<uint4*>(po.recs);
    uint32_t bin[KI], rk[KI];
#ifdef DBI_DIGEST_CLOCK  // (clock builds: the bins apart from the ranks)
#pragma unroll
    for (uint32_t k = 0; k < KI; ++k) {
        bin[k] = ~0u;
        rk[k] = 0;
        if (k * DIGEST_THREADS + tid < nr && (rv[k].x & rv[k].y) != 0xFFFFFFFFu)
            bin[k] = po.lsd ? bin_of(u4_mass(rv[k]), po.lin) : depth_bin(u4_mass(rv[k]), po.dm);
    }
    __syncthreads();
    if (clk && threadIdx.x == 0) clk[3] = __builtin_amdgcn_s_memtime();
#pragma unroll
    for (uint32_t k = 0; k < KI; ++k)
        if (bin[k] != ~0u) rk[k] = atomicAdd(&s_cnt[d1_of(bin[k])], 1u);
#else
#pragma unroll
    for (uint32_t k = 0; k < KI; ++k) {
        bin[k] = ~0u;
        rk[k] = 0;
        if (k * DIGEST_THREADS + tid < nr && (rv[k].x & rv[k].y) != 0xFFFFFFFFu) {  // not a sentinel
            bin[k] = po.lsd ? bin_of(u4_mass(rv[k]), po.lin) : depth_bin(u4_mass(rv[k]), po.dm);
            rk[k] = atomicAdd(&s_cnt[d1_of(bin[k])], 1u);
        }
    }
#endif
    __syncthreads();
    PCLK(0);
    // digit d's run: stage[lstart, lstart + c), region cursor o -> out[region(d) + o + (t - lstart)]
    const uint32_t c = tid < D1 ? s_cnt[tid] : 0u;
    uint32_t nvalid;
    const uint32_t lstart = block_excl_scan<DIGEST_THREADS, uint32_t>(c, s_tmp, nvalid);
    if (tid < D1) {
        uint32_t g = ~0u;
        if (c) {
            // the cursor is this XCD's alone (its own 1-KiB row, cur[xcd][digit]): the add runs in
            // this XCD's L2 (workgroup scope: no trip to the memory-side atomics); the kernel's end
            // writes it back.  A wrong XCD id would lose adds: k_part_plan checks the cursors' sum.
            const uint32_t o = __hip_atomic_fetch_add(&po.cur[xcd * 256u + tid], c, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_WORKGROUP);
            if (o + c <= po.cap) g = (tid * DEPTH_XCDS + xcd) * po.cap + o - lstart;
            else atomicOr(&ctr->err, ERR_PART);
        }
        s_run[tid] = g;
        s_cnt[tid] = lstart;
    }
    __syncthreads();
    PCLK(1);
#pragma unroll
    for (uint32_t k = 0; k < KI; ++k) {
        if (bin[k] != ~0u) {
            const uint32_t at = s_cnt[d1_of(bin[k])] + rk[k];
            stage[at] = rv[k];
            sdig[at] = (uint16_t)(d1_of(bin[k]) << 8 | d2_of(bin[k]));
        }
    }
    __syncthreads();
    PCLK(2);
    for (uint32_t t = tid; t < nvalid; t += DIGEST_THREADS) {
        const uint32_t bb = sdig[t];
        const uint32_t g = s_run[bb >> 8];
        if (g != ~0u) {
            out4[g + t] = stage[t];
            po.dig[g + t] = (uint8_t)(bb & 0xFFu);
        }
    }
#undef PCLK
}

template <uint32_t R>
__device__ void part_tile(const PartOut& po, const Rec* __restrict__ src, uint32_t n, uint32_t* s_cnt,
                          uint32_t* s_run, uint32_t* s_tmp, uint4* stage, uint16_t* sdig, Counters* __restrict__ ctr) {
    constexpr uint32_t KI = (R + DIGEST_THREADS - 1) / DIGEST_THREADS;
    const uint32_t tid = threadIdx.x;
    const uint4* __restrict__ src4 = reinterpret_cast<const uint4*>(src);
    // every record of the tile acknowledged by the L2 before the barrier: the
    // other waves read the slots back (from the L2: the lines were never in
    // this CU's L1).  (__threadfence() would write the L2 back to HBM per tile.)
    __builtin_amdgcn_s_waitcnt(0);
    for (uint32_t r0 = 0; r0 < n; r0 += R) {
        const uint32_t nr = min(R, n - r0);
        __syncthreads();  // the tile's slots written (first round); the last round's stage and counters read
        s_cnt[tid] = 0;
        uint4 rv[KI];
#pragma unroll
        for (uint32_t k = 0; k < KI; ++k)  // clamped: every load in flight together
            rv[k] = src4[r0 + min(k * DIGEST_THREADS + tid, nr - 1u)];
        __syncthreads();
        part_place<KI>(po, rv, nr, s_cnt, s_run, s_tmp, stage, sdig, ctr);
    }
}

#ifdef DBI_DIGEST_CLOCK  // experiment builds: summed phase cycles of the partitioning digest (dbi_debug_digest_clock)
__device__ unsigned long long g_dphase[16];
#define DPHASE(k) \
    do { if (PART && threadIdx.x == 0) dph[k] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define DPHASE(k) do { } while (0)
#endif

// H1: with the first radix histogram (Hist1; 80 VGPRs kept for 6 waves per
// SIMD, where the LDS puts the blocks).  PART: the records are partitioned by
// the depth bins' high digit afterwards (part_tile; the slots are scratch).
template <bool DROP, bool H1, bool PART = false>
__global__ void __launch_bounds__(DIGEST_THREADS) __attribute__((amdgpu_waves_per_eu(H1 || PART ? 6 : 1, 8)))
k_digest_bounded(DevParams dp, const double* __restrict__ d_mass_tab, const uint8_t* __restrict__ d_flags,
                 const uint8_t* __restrict__ d_res, const uint32_t* __restrict__ d_poff, uint32_t n_prot,
                 uint32_t n_res, const uint32_t* __restrict__ d_tile_pf, Rec* __restrict__ d_out, uint64_t cap,
                 Counters* __restrict__ d_ctr, Hist1 h1, PartOut po) {
    using SM = std::conditional_t<PART, LeanSmemP, LeanSmem>;
    __shared__ SM sm;
    __shared__ uint32_t s_kept, s_waves, s_dup;
    __shared__ unsigned long long s_base;
    __shared__ uint32_t s_h1[H1 ? H1_LDS : 1];
#ifdef DBI_DIGEST_CLOCK
    unsigned long long dph[8] = {};
#endif
    DPHASE(0);
    const uint32_t tid = threadIdx.x;
    if constexpr (H1)
        for (uint32_t i = tid; i < H1_LDS; i += DIGEST_THREADS) s_h1[i] = 0;
    if (tid == 0) {  // read at the end, behind many barriers
        s_kept = 0;
        s_waves = 0;
        s_dup = 0;
    }
    const uint32_t tile = blockIdx.x, ntiles = gridDim.x;
    const uint32_t t0 = tile * (uint32_t)DIGEST_TILE;
    const uint32_t t_end = min(t0 + (uint32_t)DIGEST_TILE, n_res);
    const uint32_t w0 = t0 >= (uint32_t)LD_PRE ? t0 - (uint32_t)LD_PRE : 0u;
    const uint32_t w_end = min(t0 + (uint32_t)(DIGEST_TILE + LD_HALO), n_res);
    const uint32_t lb = 16u + (uint32_t)((reinterpret_cast<uintptr_t>(d_res) + w0) & 15u);  // LDS position of w0
    const uint32_t lend = lb + (w_end - w0);
    const uint32_t nvec = (lend + 15u) >> 4;
    const uint8_t* __restrict__ gb = d_res + w0 - lb;  // LDS position q <- gb[q], q in [lb, lend)

    // every independent global load first: the window's 16-B vectors, the
    // tile's protein range, the tables.  The ragged first / last vector is
    // loaded whole (an aligned 16-B vector holding a byte of the residues
    // never leaves that byte's page) and the bytes outside [lb, lend) are
    // cleared: byte loads in a branch cost one HBM round trip each, and the
    // whole block waited for the wave that made them.
    constexpr uint32_t NV = (LD_WIN / 16 + DIGEST_THREADS - 1) / DIGEST_THREADS;
    uint4 rv[NV];
#pragma unroll
    for (uint32_t k = 0; k < NV; ++k) {
        const uint32_t i = tid + k * DIGEST_THREADS;
        const bool any = i < nvec && 16u * i + 16u > lb;
        rv[k] = *(any ? reinterpret_cast<const uint4*>(gb + 16u * i) : &g_zero16);
    }
    const uint32_t pf = d_tile_pf[tile], pl = d_tile_pf[ntiles + 1 + tile];
    sm.mass[tid] = d_mass_tab[tid];
    sm.flags[tid] = d_flags[tid];
    static_assert(LD_WORDS <= DIGEST_THREADS, "one thread per bit-map word");
    if (tid < (uint32_t)LD_WORDS) sm.stm[tid] = 0;
#pragma unroll
    for (uint32_t k = 0; k < NV; ++k) {
        const uint32_t i = tid + k * DIGEST_THREADS;
        const uint32_t vlo = 16u * i >= lb ? 0u : min(lb - 16u * i, 16u);
        const uint32_t vhi = 16u * i + 16u <= lend ? 16u : (lend > 16u * i ? lend - 16u * i : 0u);
        if (vlo > 0u || vhi < 16u) {  // ragged vector: keep the bytes in [lb, lend)
            uint32_t wv[4] = {rv[k].x, rv[k].y, rv[k].z, rv[k].w};
#pragma unroll
            for (uint32_t d = 0; d < 4; ++d) {
                uint32_t keep = 0;
#pragma unroll
                for (uint32_t b = 0; b < 4; ++b) keep |= (4u * d + b >= vlo && 4u * d + b < vhi) ? 0xFFu << (8 * b) : 0u;
                wv[d] &= keep;
            }
            rv[k] = make_uint4(wv[0], wv[1], wv[2], wv[3]);
        }
    }
    const uint32_t np_all = pl - pf + 2;
    const uint32_t npst = np_all <= PST_CAP ? np_all : 0u;
    uint64_t* nocm = reinterpret_cast<uint64_t*>(sm.endm());  // scratch until the walks
    uint64_t* nokm = nocm + LD_WORDS;
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(nokm + LD_WORDS);
    uint16_t* cand = sm.cand();
    __syncthreads();
    // window -> LDS, cleave / no-cut flags -> 16-bit slices of the bit maps
    // (every slice written: zeros past the window); protein starts
    for (uint32_t i = tid; i < 4u * LD_WORDS; i += DIGEST_THREADS) {
        uint32_t clv16 = 0, noc16 = 0;
        const uint32_t k = (i - tid) / DIGEST_THREADS;
        if (i < nvec) {
            const uint4 v = k == 0 ? rv[0] : rv[NV - 1];
            const uint32_t vlo = 16u * i >= lb ? 0u : lb - 16u * i;
            const uint32_t vhi = 16u * i + 16u <= lend ? 16u : lend - 16u * i;
            const uint32_t valid = (vhi > vlo) ? ((1u << vhi) - 1u) & ~((1u << vlo) - 1u) : 0u;
            const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
            uint32_t ptm16 = 0;
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const uint32_t f = sm.flags[(wv[b >> 2] >> (8 * (b & 3))) & 0xFFu];
                clv16 |= (f & F_CLEAVE) << b;
                noc16 |= ((f >> 1) & 1u) << b;
                ptm16 |= ((f >> 5) & 1u) << b;
            }
            static_assert(F_CLEAVE == 1 && F_NOCUT == 2 && F_PTM == 32, "flag bits");
            clv16 &= valid;
            noc16 &= valid;
            if (ptm16 & valid) atomicOr(&d_ctr->err, ERR_PTM);  // '[' in device input
            reinterpret_cast<uint4*>(sm.win)[i] = v;
        }
        reinterpret_cast<uint16_t*>(sm.clvm)[i] = (uint16_t)clv16;
        reinterpret_cast<uint16_t*>(nocm)[i] = (uint16_t)noc16;
    }
    static_assert(NV == 2 && (4 * LD_WORDS) <= 2 * DIGEST_THREADS, "two vectors per thread");
    for (uint32_t i = tid; i < np_all; i += DIGEST_THREADS) {
        const uint32_t o = d_poff[pf + i];
        if (o >= w0 && o <= w_end) {
            const uint32_t q = o - w0 + lb;  // protein starts (and the end of the last one)
            const uint64_t bit = 1ull << (q & 63);
            if (atomicOr(&sm.stm[q >> 6], bit) & bit) s_dup = 1;  // an empty protein: two starts at q
        }
        if (i < PST_CAP) sm.pst[i] = o;
    }
    __syncthreads();
    // protein of a start from the start map: the marked starts before its word
    // (one wave's scan) + those up to it in the word.  Not when two proteins
    // start at one position (empty proteins) or the offsets did not fit pst.
    const bool pid_map = npst != 0 && s_dup == 0;  // block-uniform
    if (pid_map && tid < 64) {
        static_assert(LD_WORDS <= 128, "two words per lane");
        const uint32_t c0 = 2 * tid < (uint32_t)LD_WORDS ? (uint32_t)__popcll(sm.stm[2 * tid]) : 0u;
        const uint32_t c1 = 2 * tid + 1 < (uint32_t)LD_WORDS ? (uint32_t)__popcll(sm.stm[2 * tid + 1]) : 0u;
        const uint32_t ex = wave_incl_scan(c0 + c1) - (c0 + c1);
        if (2 * tid < (uint32_t)LD_WORDS) sm.wpre[2 * tid] = (uint16_t)ex;
        if (2 * tid + 1 < (uint32_t)LD_WORDS) sm.wpre[2 * tid + 1] = (uint16_t)(ex + c0);
    }
    // poff[pf] <= t0 always; it is marked unless it lies before the window
    const uint32_t pid_base = pf + (npst != 0 && sm.pst[0] < w0 ? 1u : 0u) - 1u;
    // cut and N_ok maps, 64 positions per thread from the bit maps:
    //   last     = a protein starts at q+1
    //   cut      = last || (cleave(q) && !nocut(q+1))        (checkCleavage C side)
    //   cut_prev = cleave(q-1) && !nocut(q)                   (its protein-end case is a start)
    //   N_ok     = start(q) || cut_prev                       (the candidate starts)
    // The window's last position (w_end < R): the next residue is unknown, its
    // cut bit is never used (lean_ends' `known`).
    if (tid < (uint32_t)LD_WORDS) {
        const uint32_t w = tid;
        const uint64_t valid = low_bits(lend > 64u * w ? min(lend - 64u * w, 64u) : 0u) &
                               ~low_bits(lb > 64u * w ? min(lb - 64u * w, 64u) : 0u);
        const uint64_t st = sm.stm[w];
        const uint64_t st_n = w + 1 < (uint32_t)LD_WORDS ? sm.stm[w + 1] : 0ull;
        const uint64_t cl = sm.clvm[w];
        const uint64_t cl_p = w > 0 ? sm.clvm[w - 1] : 0ull;
        const uint64_t nc = nocm[w];
        const uint64_t nc_n = w + 1 < (uint32_t)LD_WORDS ? nocm[w + 1] : 0ull;
        const uint64_t lastm = (st >> 1) | (st_n << 63);
        sm.cutm[w] = (lastm | (cl & ~((nc >> 1) | (nc_n << 63)))) & valid;
        nokm[w] = (st | (((cl << 1) | (cl_p >> 63)) & ~nc)) & valid;
    }
    __syncthreads();
    DPHASE(1);
    // cleavage-site compaction: thread t owns starts [16t, 16t+16) of the tile, in order
    const uint32_t off = lb + (t0 - w0);  // LDS position of the tile's first start
    const uint32_t n_here = t0 + tid * STARTS_PER_THREAD < t_end
                                ? min((uint32_t)STARTS_PER_THREAD, t_end - t0 - tid * STARTS_PER_THREAD) : 0u;
    const uint32_t mybits = (uint32_t)bits_from(nokm, off + tid * STARTS_PER_THREAD) &
                            (n_here >= 16 ? 0xFFFFu : ((1u << n_here) - 1u));
    uint32_t ncand;
    uint32_t pos = block_excl_scan<DIGEST_THREADS, uint32_t>((uint32_t)__popc(mybits), sm.tmp, ncand);
#pragma unroll
    for (int k = 0; k < STARTS_PER_THREAD; ++k)
        if (mybits & (1u << k)) cand[pos++] = (uint16_t)(tid * STARTS_PER_THREAD + k);
    __syncthreads();

    const uint32_t B = (uint32_t)dp.max_missed + 2u;  // records per start, at most
    const uint32_t min_len = (uint32_t)dp.min_len;
    const uint32_t known = w_end == n_res ? lend - 1u : lend - 2u;
    const uint32_t max_plen = d_ctr->max_plen;
    const uint32_t w = rec_width(max_plen);
    if (tile == 0 && tid == 0 && !rec_layout_ok(w, n_prot)) atomicOr(&d_ctr->err, ERR_LAYOUT);
    balance_candidates(cand, s_cnt, ncand, B, t_end - t0);
    DPHASE(2);
    uint32_t jb, je;
    thread_share(ncand, jb, je);
    // slot bounds: the candidate ends (B for a walk that may leave the horizon);
    // the first two starts' ends stay in registers for the walks (most threads
    // have one or two: ncand ~ 450 per tile)
    uint32_t lim = 0;
    LeanEnds en0{0ull, 0ull, 0u, false}, en1{0ull, 0ull, 0u, false};
    for (uint32_t j = jb; j < je; ++j) {
        const LeanEnds en = lean_ends(sm, off + cand[j], known, B, min_len);
        if (j == jb) en0 = en;
        else if (j == jb + 1) en1 = en;
        lim += en.open ? B : (uint32_t)(__popcll(en.lo) + __popcll(en.hi));
    }
    uint32_t tile_slots;
    const uint32_t excl_t = block_excl_scan<DIGEST_THREADS, uint32_t>(lim, sm.tmp, tile_slots);
    // PART stage mode (block-uniform): the tile's records stay in LDS, 12 B
    // each behind the candidate list (smass / sinfo, slot excl_t + k of each
    // thread as in d_out), until part_place writes them into the regions --
    // no slot of d_out is written or read back.  A tile whose slot bound does
    // not fit (or a proteome with proteins of 2^20 residues) takes the slots.
    constexpr uint32_t PR = PART ? (uint32_t)((sizeof(SM) - offsetof(SM, clvm)) / 18 / 64 * 64) : 64u;
    bool stage = false;
    double* smass = nullptr;
    uint32_t* sinfo = nullptr;
    if constexpr (PART) {
        const uint32_t c16 = (2u * ncand + 15u) & ~15u;
        const uint32_t room = (LD_POOL_PART - c16) / 12u;
        stage = po.stage && tile_slots <= min(room, PR) && (max_plen >> STAGE_LEN_BITS) == 0;
        smass = reinterpret_cast<double*>(sm.pool + c16);
        sinfo = reinterpret_cast<uint32_t*>(sm.pool + c16 + 8u * room);
    }
    // the tile's output region: one atomic add, in whatever order the tiles
    // get here (no tile waits for another; the chunk sort does not need
    // records in first-appearance order, ck_fix_runs); ctr->n_slots ends as
    // the total.  A staged tile takes none: its records never touch d_out
    // (n_slots counts the slots of the tiles that did; one contended device
    // atomic and a barrier's wait for it fewer per tile)
    unsigned long long base = 0;
    if (!stage) {
        if (tid == 0) s_base = atomicAdd(&d_ctr->n_slots, (unsigned long long)tile_slots);
        __syncthreads();
        base = s_base;
        if (base + tile_slots > cap) return;  // too small: the caller grows it and runs again
    }
    DPHASE(3);

    Rec* __restrict__ o = d_out + base + excl_t;
    const uint32_t c0 = (uint32_t)(base / RADIX_CHUNK_D);
    // the protein of the start at LDS position p (global index s) and its first residue
    auto protein_at = [&](uint32_t p, uint32_t s, uint32_t& pstart) {
        uint32_t pid;
        if (pid_map) {
            pid = pid_base + sm.wpre[p >> 6] + (uint32_t)__popcll(sm.stm[p >> 6] & low_bits((p & 63u) + 1u));
            pstart = sm.pst[pid - pf];
        } else {
            pid = protein_of(sm.pst, npst, pf, pl, d_poff, s, pstart);
        }
        return pid;
    };
    uint32_t kept = 0, dropped = 0;
    for (uint32_t j = jb; j < je; ++j) {
        const uint32_t p = off + cand[j];
        const uint32_t s = w0 + (p - lb);
        double* em = PART && stage ? smass + excl_t + kept : sm.endm() + tid;
        const LeanWalk lw = lean_masses(dp, sm, p, j == jb ? en0 : j == jb + 1 ? en1 : lean_ends(sm, p, known, B, min_len),
                                        em, PART && stage ? 1u : (uint32_t)DIGEST_THREADS);
        WalkOut wo;
        if (PART && stage) {
            if (lw.overflow) {
                uint32_t pstart;
                const uint32_t pe = d_poff[protein_at(p, s, pstart) + 1];
                wo = walk_global_to<true, false, false>(dp, sm.mass, sm.flags, d_res, s, pe, true,
                                                        StageSink{em, sinfo + excl_t + kept, j, lim - kept});
            } else {
                wo = lean_stage<DROP>(dp, lw, em, sinfo + excl_t + kept, j);
            }
        } else {
            uint32_t pstart;
            const uint32_t pid = protein_at(p, s, pstart);
            const uint64_t loc = rec_loc(pid, s - pstart, w);
            if (lw.overflow) {
                const uint32_t pe = d_poff[pid + 1];
                wo = walk_global<true, false, false>(dp, sm.mass, sm.flags, d_res, s, pe, true, loc, o + kept, o + lim);
                if constexpr (H1)  // rare: the records it wrote, read back
                    for (uint32_t k = kept; k < kept + wo.kept; ++k)
                        hist1_count(h1, s_h1, c0, q0_mass(o[k].q0), (uint32_t)base + excl_t + k);
            } else {
                wo = lean_emit<DROP, H1>(dp, sm, p, lw, em, loc, o + kept, h1, s_h1, c0,
                                         (uint32_t)base + excl_t + kept);
            }
        }
        kept += wo.kept;
        dropped += wo.dropped;
    }
    if (kept > lim) atomicOr(&d_ctr->err, ERR_SLOTS);  // the bound is an upper bound: never
    if (PART && stage) {
        for (uint32_t k = kept; k < lim; ++k) sinfo[excl_t + k] = STAGE_NONE;
    } else {
        const Rec sent{REC_SENTINEL, REC_SENTINEL};
        for (uint32_t k = kept; k < lim; ++k) o[k] = sent;
    }
    bool flush;
    if (DROP) {
        const uint32_t tk = block_sum<DIGEST_THREADS, uint32_t>(kept, sm.tmp);
        const uint32_t td = block_sum<DIGEST_THREADS, uint32_t>(dropped, sm.tmp);
        if (tid == 0) {
            if (tk) atomicAdd(&d_ctr->n_kept, (unsigned long long)tk);
            if (td) atomicAdd(&d_ctr->n_dropped, (unsigned long long)td);
        }
        flush = tid < 64;  // behind the block sums' barriers
    } else {
        // nothing is dropped (drop_mass > maxMH, also in walk_global); the tile
        // total without a barrier: each wave adds its sum in LDS, the last wave
        // to arrive publishes it (and flushes the histogram counters)
        const uint32_t wk = wave_sum(kept);
        uint32_t last = 0;
        if (lane_id() == 0) {
            atomicAdd(&s_kept, wk);
            __threadfence_block();
            if (atomicAdd(&s_waves, 1u) == DIGEST_THREADS / 64 - 1) {
                last = 1;
                const uint32_t tk = atomicAdd(&s_kept, 0u);
                if (tk) atomicAdd(&d_ctr->n_kept, (unsigned long long)tk);
            }
        }
        flush = __builtin_amdgcn_readlane((int)last, 0) != 0;
    }
    if (H1 && flush) {
        __threadfence_block();
        for (uint32_t i = lane_id(); i < H1_LDS; i += 64) {
            const uint32_t v = atomicAdd(&s_h1[i], 0u), c = c0 + (i >> h1.bits);
            if (v && c < h1.G) atomicAdd(&h1.g[(size_t)(i & ((1u << h1.bits) - 1u)) * h1.G + c], v);
        }
    }
    if constexpr (PART) {  // the walks' LDS is dead: the partition's counters and stage
        constexpr size_t b0 = offsetof(SM, clvm);
        static_assert(b0 % 16 == 0 && PR >= 1024, "partition stage");
        uint8_t* st = reinterpret_cast<uint8_t*>(&sm) + b0;
        uint32_t* p_cnt = reinterpret_cast<uint32_t*>(sm.mass);
        if (stage) {
            // every record rebuilt from its 12 B and the window: the tag from the
            // peptide's end bytes (HBM past the window: walk_global's long ones),
            // the protein and offset from the start's candidate index
            constexpr uint32_t KS = (PR + DIGEST_THREADS - 1) / DIGEST_THREADS;
            __syncthreads();  // every walk's records staged, the walks' mass-table reads done
            DPHASE(4);
            p_cnt[tid] = 0;
            const uint32_t* __restrict__ w32 = reinterpret_cast<const uint32_t*>(sm.win);
            uint4 rr[KS];
#pragma unroll
            for (uint32_t k = 0; k < KS; ++k) {
                const uint32_t i = k * DIGEST_THREADS + tid;
                rr[k] = make_uint4(~0u, ~0u, ~0u, ~0u);
                const uint32_t info = i < tile_slots ? sinfo[i] : STAGE_NONE;
                if (info != STAGE_NONE) {
                    const double m = smass[i];
                    const uint32_t len = info & ((1u << STAGE_LEN_BITS) - 1u);
                    const uint32_t p = off + cand[info >> STAGE_LEN_BITS];
                    const uint32_t s = w0 + (p - lb);
                    uint32_t pstart;
                    const uint32_t pid = protein_at(p, s, pstart);
                    const uint32_t head = __builtin_amdgcn_alignbyte(w32[(p >> 2) + 1], w32[p >> 2], p & 3u);
                    uint32_t tail = 0;
                    if (p + len - 1u <= known) {
                        const uint32_t q = p + len - 4u;  // p >= 16
                        tail = __builtin_bswap32(__builtin_amdgcn_alignbyte(w32[(q >> 2) + 1], w32[q >> 2], q & 3u));
                    } else {
                        for (uint32_t b = 0; b < 4 && b < len; ++b) tail |= (uint32_t)d_res[s + len - 1u - b] << (8 * b);
                    }
                    const uint32_t tag = peptide_tag(head, tail, len);
                    const uint64_t q0 = rec_q0(m, tag), q1 = rec_q1(tag, rec_loc(pid, s - pstart, w), len);
                    rr[k] = make_uint4((uint32_t)q0, (uint32_t)(q0 >> 32), (uint32_t)q1, (uint32_t)(q1 >> 32));
                }
            }
            __syncthreads();  // the stage, list and window read: part_place's stage overwrites them
            DPHASE(5);
#ifdef DBI_DIGEST_CLOCK
            unsigned long long pcl[4] = {};
            part_place<KS>(po, rr, tile_slots, p_cnt, p_cnt + 256, sm.tmp, reinterpret_cast<uint4*>(st),
                           reinterpret_cast<uint16_t*>(st + 16 * PR), d_ctr, pcl);
#else
            part_place<KS>(po, rr, tile_slots, p_cnt, p_cnt + 256, sm.tmp, reinterpret_cast<uint4*>(st),
                           reinterpret_cast<uint16_t*>(st + 16 * PR), d_ctr);
#endif
#ifdef DBI_DIGEST_CLOCK
            __syncthreads();
            DPHASE(6);
            if (threadIdx.x == 0) {
                atomicAdd(&g_dphase[11], pcl[0] - dph[5]);   // bins + ranks
                atomicAdd(&g_dphase[15], pcl[3] - dph[5]);   // bins alone
                atomicAdd(&g_dphase[12], pcl[1] - pcl[0]);   // scan + region reservation
                atomicAdd(&g_dphase[13], pcl[2] - pcl[1]);   // restage in digit order
                atomicAdd(&g_dphase[14], dph[6] - pcl[2]);   // runs written
                for (int k = 0; k < 6; ++k) atomicAdd(&g_dphase[k], dph[k + 1] - dph[k]);
                atomicAdd(&g_dphase[8], 1ull);
                atomicAdd(&g_dphase[9], (unsigned long long)tile_slots);
                atomicAdd(&g_dphase[10], (unsigned long long)ncand);
            }
#endif
        } else {
            part_tile<PR>(po, d_out + base, tile_slots, p_cnt, p_cnt + 256, sm.tmp, reinterpret_cast<uint4*>(st),
                          reinterpret_cast<uint16_t*>(st + 16 * PR), d_ctr);
        }
    }
}

hipError_t launch_digest_bounded(const DevParams& dp, const double* d_mass_tab, const uint8_t* d_flags,
                                 const uint8_t* d_res, const uint32_t* d_poff, uint32_t n_prot, uint32_t n_res,
                                 const uint32_t* d_tile_pf, Rec* d_out, uint64_t cap, Counters* d_ctr, hipStream_t s,
                                 const Hist1Plan* h1p, const PartOut* part) {
    const uint32_t nblk = (n_res + DIGEST_TILE - 1) / DIGEST_TILE;
    if (nblk == 0) return hipSuccess;
    if (dp.semi || dp.mand_mode || dp.max_missed + 2 > LD_ENDS) return hipErrorInvalidValue;
    Hist1 h1{nullptr, BinMap{}, 0u, 0u};
    if (h1p) {
        if (h1p->bits < 1 || h1p->bits > RADIX_BITS || (uint64_t)h1p->G * RADIX_CHUNK_D < cap) return hipErrorInvalidValue;
        h1 = Hist1{h1p->hist, h1p->bm, (uint32_t)h1p->bits, h1p->G};
    }
    PartOut po{};
    if (part) {
        if (h1p || part->b1 < 1 || part->b1 > 8 || part->dm.b2 < 1 || part->dm.b2 > RADIX_BITS || part->cap % 64)
            return hipErrorInvalidValue;
        po = *part;
    }
#define DBI_DIGEST_B(DROP, H1, PART)                                                                                \
    DBI_LAUNCH((k_digest_bounded<DROP, H1, PART>), dim3(nblk), dim3(DIGEST_THREADS), 0, s, dp, d_mass_tab, d_flags, \
               d_res, d_poff, n_prot, n_res, d_tile_pf, d_out, cap, d_ctr, h1, po)
    const bool drop = dp.drop_mass <= dp.max_mh;
    if (part) {
        if (drop) DBI_DIGEST_B(true, false, true);
        else DBI_DIGEST_B(false, false, true);
    } else if (h1p) {
        if (drop) DBI_DIGEST_B(true, true, false);
        else DBI_DIGEST_B(false, true, false);
    } else {
        if (drop) DBI_DIGEST_B(true, false, false);
        else DBI_DIGEST_B(false, false, false);
    }
#undef DBI_DIGEST_B
    return hipGetLastError();
}

// the bucket count's tracked-boundary kernel applies: NUM_BUCKETS <= 8,
// its thresholds compare in u32 ([3, 2^31)), and the first end of a start is
// past window position 0 (MIN_PEP_LENGTH >= 2)
static bool count_fast_ok(const DevParams& dp) {
    return dp.nb >= 1 && dp.nb <= HIST_FAST_MAX && dp.min_len >= 2 && cut_threshold((double)dp.br, dp.m0) >= CUT_EPS_FX &&
           cut_threshold((double)(dp.nb * dp.br), dp.m0) < (1ll << 31);
}

// the tracked boundaries' count k1 - k0, as k_digest_count_cuts derives k0 / k1
// from the same thresholds (cut_threshold: host and device)
static int count_tracked(const DevParams& dp) {
    const int64_t t_min = cut_threshold(dp.min_mh, dp.m0), t_max = cut_threshold(dp.max_mh, dp.m0);
    int k0 = 0, k1 = 0;
    for (int k = 0; k < HIST_FAST_MAX; ++k) {
        const int64_t tb = cut_threshold((double)((k + 1) * dp.br), dp.m0);
        if (k < dp.nb && tb <= t_min) k0 = k + 1;
        if (k < dp.nb && tb < t_max) k1 = k + 1;
    }
    return std::max(0, k1 - k0);
}

template <bool EMIT, bool HIST = false>
static hipError_t launch_digest(const DevParams& dp, const double* d_mass_tab, const uint8_t* d_flags,
                                const uint8_t* d_res, const uint32_t* d_poff, uint32_t n_prot, uint32_t n_res,
                                const uint32_t* d_tile_pf, uint32_t* d_blk, uint32_t* d_thr, Rec* d_out,
                                Counters* d_ctr, hipStream_t s, unsigned long long* d_hist = nullptr) {
    const uint32_t nblk = (n_res + DIGEST_TILE - 1) / DIGEST_TILE;
    if (nblk == 0) return hipSuccess;
    static_assert(!EMIT || !HIST, "bucket counts come from COUNT passes");
#define DBI_DIGEST(SEMI, MAND)                                                                                   \
    do {                                                                                                         \
        if (dp.pf_kind)                                                                                          \
            DBI_LAUNCH((k_digest<EMIT, SEMI, MAND, HIST, true>), dim3(nblk), dim3(DIGEST_THREADS), 0, s, dp,     \
                       d_mass_tab, d_flags, d_res, d_poff, n_prot, n_res, d_tile_pf, d_blk, d_thr, d_out, d_ctr, \
                       d_hist);                                                                                  \
        else                                                                                                     \
            DBI_LAUNCH((k_digest<EMIT, SEMI, MAND, HIST>), dim3(nblk), dim3(DIGEST_THREADS), 0, s, dp,           \
                       d_mass_tab, d_flags, d_res, d_poff, n_prot, n_res, d_tile_pf, d_blk, d_thr, d_out, d_ctr, \
                       d_hist);                                                                                  \
    } while (0)
    if (!EMIT && !dp.semi && !dp.mand_mode && dp.cut_count && !dp.pf_kind) {
        if (HIST && count_fast_ok(dp)) {
#define DBI_COUNT_KT(KT)                                                                                   \
    DBI_LAUNCH((k_digest_count_cuts<HIST, true, KT>), dim3(nblk), dim3(DIGEST_THREADS), 0, s, dp, d_mass_tab, \
               d_flags, d_res, d_poff, n_prot, n_res, d_tile_pf, d_blk, d_thr, d_ctr, d_hist)
            switch (count_tracked(dp)) {
            case 0: DBI_COUNT_KT(0); break;
            case 1: DBI_COUNT_KT(1); break;
            case 2: DBI_COUNT_KT(2); break;
            case 3: DBI_COUNT_KT(3); break;
            case 4: DBI_COUNT_KT(4); break;
            case 5: DBI_COUNT_KT(5); break;
            case 6: DBI_COUNT_KT(6); break;
            case 7: DBI_COUNT_KT(7); break;
            default: DBI_COUNT_KT(8); break;
            }
#undef DBI_COUNT_KT
        } else
            DBI_LAUNCH(k_digest_count_cuts<HIST>, dim3(nblk), dim3(DIGEST_THREADS), 0, s, dp, d_mass_tab, d_flags,
                       d_res, d_poff, n_prot, n_res, d_tile_pf, d_blk, d_thr, d_ctr, d_hist);
        return hipGetLastError();
    }
    if (dp.semi) {
        if (dp.mand_mode) DBI_DIGEST(true, true); else DBI_DIGEST(true, false);
    } else {
        if (dp.mand_mode) DBI_DIGEST(false, true); else DBI_DIGEST(false, false);
    }
#undef DBI_DIGEST
    return hipGetLastError();
}

hipError_t launch_digest_count(const DevParams& dp, const double* d_mass_tab, const uint8_t* d_flags,
                               const uint8_t* d_res, const uint32_t* d_poff, uint32_t n_prot,
                               uint32_t n_res, const uint32_t* d_tile_pf, uint32_t* d_blk, uint32_t* d_thr,
                               Counters* d_ctr, hipStream_t s) {
    return launch_digest<false>(dp, d_mass_tab, d_flags, d_res, d_poff, n_prot, n_res, d_tile_pf, d_blk, d_thr,
                                nullptr, d_ctr, s);
}

hipError_t launch_digest_count_hist(const DevParams& dp, const double* d_mass_tab, const uint8_t* d_flags,
                                    const uint8_t* d_res, const uint32_t* d_poff, uint32_t n_prot, uint32_t n_res,
                                    const uint32_t* d_tile_pf, uint32_t* d_blk, uint32_t* d_thr, Counters* d_ctr,
                                    unsigned long long* d_hist, hipStream_t s) {
    if (dp.nb < 1 || dp.nb > HIST_MAX_BUCKETS) return hipErrorInvalidValue;
    return launch_digest<false, true>(dp, d_mass_tab, d_flags, d_res, d_poff, n_prot, n_res, d_tile_pf, d_blk, d_thr,
                                      nullptr, d_ctr, s, d_hist);
}

hipError_t launch_digest_emit(const DevParams& dp, const double* d_mass_tab, const uint8_t* d_flags,
                              const uint8_t* d_res, const uint32_t* d_poff, uint32_t n_prot,
                              uint32_t n_res, const uint32_t* d_tile_pf, uint32_t* d_blk_off, uint32_t* d_thr,
                              Rec* d_out, Counters* d_ctr, hipStream_t s) {
    return launch_digest<true>(dp, d_mass_tab, d_flags, d_res, d_poff, n_prot, n_res, d_tile_pf, d_blk_off, d_thr,
                               d_out, d_ctr, s);
}

// ---------------------------------------------------------------------------
// 2. exclusive scan of u32 (reduce -> single-block scan of block sums -> downsweep)
// ---------------------------------------------------------------------------
constexpr int SCAN_THREADS = 1024;
constexpr int SCAN_ITEMS = 4;
constexpr uint64_t SCAN_CHUNK = (uint64_t)SCAN_THREADS * SCAN_ITEMS;

__global__ void __launch_bounds__(SCAN_THREADS)
k_scan_reduce(const uint32_t* __restrict__ in, uint64_t n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t tmp[SCAN_THREADS / 64 + 1];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_CHUNK;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const uint64_t i = base + (uint64_t)k * SCAN_THREADS + threadIdx.x;
        if (i < n) v += in[i];
    }
    const uint32_t t = block_sum<SCAN_THREADS, uint32_t>(v, tmp);
    if (threadIdx.x == 0) sums[blockIdx.x] = t;
}

// single block: exclusive scan of n values in place-able, u64 carry, total -> *d_total
__global__ void __launch_bounds__(SCAN_THREADS)
k_scan_single(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n,
              unsigned long long* __restrict__ d_total) {
    __shared__ unsigned long long tmp[SCAN_THREADS / 64 + 1];
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n; base += SCAN_CHUNK) {
        uint32_t v[SCAN_ITEMS];
        unsigned long long loc = 0;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            const uint64_t i = base + (uint64_t)threadIdx.x * SCAN_ITEMS + k;
            v[k] = i < n ? in[i] : 0u;
            loc += v[k];
        }
        unsigned long long tot;
        unsigned long long run = block_excl_scan<SCAN_THREADS, unsigned long long>(loc, tmp, tot);
        run += carry;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            const uint64_t i = base + (uint64_t)threadIdx.x * SCAN_ITEMS + k;
            if (i < n) out[i] = (uint32_t)run;
            run += v[k];
        }
        carry += tot;
    }
    if (threadIdx.x == 0 && d_total) *d_total = carry;
}

__global__ void __launch_bounds__(SCAN_THREADS)
k_scan_down(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n,
            const uint32_t* __restrict__ block_off) {
    __shared__ uint32_t tmp[SCAN_THREADS / 64 + 1];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_CHUNK;
    uint32_t v[SCAN_ITEMS];
    uint32_t loc = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const uint64_t i = base + (uint64_t)threadIdx.x * SCAN_ITEMS + k;
        v[k] = i < n ? in[i] : 0u;
        loc += v[k];
    }
    uint32_t tot;
    uint32_t run = block_excl_scan<SCAN_THREADS, uint32_t>(loc, tmp, tot) + block_off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const uint64_t i = base + (uint64_t)threadIdx.x * SCAN_ITEMS + k;
        if (i < n) out[i] = run;
        run += v[k];
    }
}

// Downsweep that finds its own block offset: the sum of the block sums before
// it (nb <= SCAN_SELF_MAX, read by every block from L2), so the scan is two
// launches instead of three.  The last block writes the total.
constexpr uint64_t SCAN_SELF_MAX = SCAN_CHUNK;

__global__ void __launch_bounds__(SCAN_THREADS)
k_scan_down_self(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n,
                 const uint32_t* __restrict__ sums, unsigned long long* __restrict__ d_total) {
    __shared__ unsigned long long tmp[SCAN_THREADS / 64 + 1];
    __shared__ uint32_t tmp32[SCAN_THREADS / 64 + 1];
    const uint32_t b = blockIdx.x;
    unsigned long long before = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const uint32_t i = (uint32_t)k * SCAN_THREADS + threadIdx.x;
        if (i < b) before += sums[i];
    }
    before = block_sum<SCAN_THREADS, unsigned long long>(before, tmp);
    const uint64_t base = (uint64_t)b * SCAN_CHUNK;
    uint32_t v[SCAN_ITEMS];
    uint32_t loc = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const uint64_t i = base + (uint64_t)threadIdx.x * SCAN_ITEMS + k;
        v[k] = i < n ? in[i] : 0u;
        loc += v[k];
    }
    uint32_t tot;
    uint32_t run = block_excl_scan<SCAN_THREADS, uint32_t>(loc, tmp32, tot) + (uint32_t)before;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const uint64_t i = base + (uint64_t)threadIdx.x * SCAN_ITEMS + k;
        if (i < n) out[i] = run;
        run += v[k];
    }
    if (d_total && b + 1 == gridDim.x && threadIdx.x == 0) *d_total = before + tot;
}

size_t scan_u32_tmp_elems(uint64_t n) { return (size_t)((n + SCAN_CHUNK - 1) / SCAN_CHUNK) + 1; }

hipError_t launch_scan_u32(const uint32_t* d_in, uint32_t* d_out, uint64_t n, uint32_t* d_block_tmp,
                           uint64_t tmp_elems, unsigned long long* d_total, hipStream_t s) {
    if (n <= SCAN_CHUNK * 4) {
        DBI_LAUNCH(k_scan_single, dim3(1), dim3(SCAN_THREADS), 0, s, d_in, d_out, n, d_total);
        return hipGetLastError();
    }
    const uint64_t nb = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
    if (tmp_elems < nb) return hipErrorInvalidValue;
    if (nb <= SCAN_SELF_MAX) {
        DBI_LAUNCH(k_scan_reduce, dim3((uint32_t)nb), dim3(SCAN_THREADS), 0, s, d_in, n, d_block_tmp);
        DBI_LAUNCH(k_scan_down_self, dim3((uint32_t)nb), dim3(SCAN_THREADS), 0, s, d_in, d_out, n, d_block_tmp,
                   d_total);
        return hipGetLastError();
    }
    DBI_LAUNCH(k_scan_reduce, dim3((uint32_t)nb), dim3(SCAN_THREADS), 0, s, d_in, n, d_block_tmp);
    DBI_LAUNCH(k_scan_single, dim3(1), dim3(SCAN_THREADS), 0, s, d_block_tmp, d_block_tmp, nb, d_total);
    DBI_LAUNCH(k_scan_down, dim3((uint32_t)nb), dim3(SCAN_THREADS), 0, s, d_in, d_out, n, d_block_tmp);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 4. stable LSD radix pass over the mass-bin id (digit = (bin >> shift) & mask)
// ---------------------------------------------------------------------------
constexpr uint32_t RADIX_CHUNK = RADIX_THREADS * RADIX_ITEMS;
constexpr int RADIX_D = 1 << RADIX_BITS;
constexpr int RADIX_NW = RADIX_THREADS / 64;

size_t radix_hist_elems(uint32_t n, int bits) {
    const uint64_t g = (n + RADIX_CHUNK - 1) / RADIX_CHUNK;
    return (size_t)g * (size_t)(1u << bits);
}

// Digit policies of a stable pass: the digit of a record from its first word
// q0, and what happens to the record on its way out.
struct BinDigit {  // LSD radix over the fine mass bin: (bin >> shift) & mask
    BinMap bm;
    int shift;
    uint32_t mask;
    __device__ __forceinline__ uint32_t operator()(uint64_t q0) const {
        return (bin_of(q0_mass(q0), bm) >> shift) & mask;
    }
    // the digit of the same record in the next pass (written next to it)
    __device__ __forceinline__ uint32_t next(uint64_t q0, int nshift, uint32_t nmask) const {
        return (bin_of(q0_mass(q0), bm) >> nshift) & nmask;
    }
    // this pass's digit | the next pass's << 8, from one bin computation
    __device__ __forceinline__ uint32_t both(uint64_t q0, int nshift, uint32_t nmask) const {
        const uint32_t b = bin_of(q0_mass(q0), bm);
        return ((b >> shift) & mask) | (((b >> nshift) & nmask) << 8);
    }
    __device__ __forceinline__ void xform(uint4&) const {}
};
struct OwnerDigit {  // owner shard: number of splitter keys <= (int)(m * factor)
    OwnerMap om;
    __device__ __forceinline__ uint32_t operator()(uint64_t q0) const {
        const int32_t k = java_d2i(q0_mass(q0) * (double)om.factor);
        uint32_t d = 0;
        for (uint32_t j = 0; j + 1 < om.nshards; ++j) d += k >= om.split[j] ? 1u : 0u;
        return d;
    }
    __device__ __forceinline__ uint32_t next(uint64_t, int, uint32_t) const { return 0u; }
    __device__ __forceinline__ uint32_t both(uint64_t q0, int, uint32_t) const { return (*this)(q0); }
    __device__ __forceinline__ void xform(uint4& r) const {  // local -> global protein id
        const uint64_t q1 = u4_q1(r) + om.pid_add;
        r.z = (uint32_t)q1;
        r.w = (uint32_t)(q1 >> 32);
    }
};
struct PairDigit {  // query routing pairs: q0 = owner shard, q1 = query index
    __device__ __forceinline__ uint32_t operator()(uint64_t q0) const { return (uint32_t)q0; }
    __device__ __forceinline__ uint32_t next(uint64_t, int, uint32_t) const { return 0u; }
    __device__ __forceinline__ uint32_t both(uint64_t q0, int, uint32_t) const { return (uint32_t)q0 & 0xFFu; }
    __device__ __forceinline__ void xform(uint4&) const {}
};

// The record chunk of this block.  Workgroups go to the 8 XCDs round-robin
// (block b on XCD b % 8), so each XCD takes one contiguous run of chunks: the
// digit runs that consecutive chunks write next to each other (their (digit,
// chunk) offsets are adjacent) meet in one L2, which merges the partial lines,
// and the 32 chunks sharing a 128-B line of a histogram row are one XCD's.
// SwissProt scatter 1.49 -> 1.24 ms per build (semi-tryptic 29.0 -> 27.3).
__device__ __forceinline__ uint32_t xcd_contiguous_block() {
    const uint32_t G = gridDim.x, b = blockIdx.x, x = b & 7u, q = G >> 3, r = G & 7u;
    return x * q + min(x, r) + (b >> 3);
}
// (Not for the chunk sort or finalize: mass-adjacent chunks cost alike, and
// one XCD per contiguous run of them loses the balance: 0.87 -> 1.10 ms and
// 0.44 -> 0.47 ms.)
__device__ __forceinline__ uint32_t radix_chunk() { return xcd_contiguous_block(); }

// Digit of record r for this pass, and the wave's peers holding the same digit.
__device__ __forceinline__ uint64_t digit_peers(uint32_t d, bool valid, int bits) {
    uint64_t peers = __ballot(valid);
    for (int b = 0; b < bits; ++b) {
        const uint64_t bal = __ballot((d >> b) & 1u);
        peers &= ((d >> b) & 1u) ? bal : ~bal;
    }
    return peers;
}

// Wave w of a block owns the contiguous records [base + w*RADIX_ITEMS*64,
// +RADIX_ITEMS*64), item k = lanes' records k*64 + lane: per-wave digit counts
// accumulate in input order, so ranks are stable with no block barrier inside
// the item loop.
template <bool SPARSE, typename Digit>
__global__ void __launch_bounds__(RADIX_THREADS)
k_radix_hist(const Rec* __restrict__ in, uint32_t n, Digit dig, int bits, uint32_t* __restrict__ hist,
             const unsigned long long* __restrict__ dn) {
    __shared__ uint32_t cnt[RADIX_NW][RADIX_D];
    if (dn) n = (uint32_t)min((unsigned long long)n, *dn);  // device-sized build: the count on the device
    const uint32_t D = 1u << bits;
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    for (uint32_t d = lane; d < D; d += 64) cnt[w][d] = 0;
    wave_sync();
    const uint32_t cb = radix_chunk();
    const uint32_t base = cb * RADIX_CHUNK + w * (RADIX_ITEMS * 64);
    uint64_t qv[RADIX_ITEMS];
    if (base + RADIX_ITEMS * 64 <= n) {  // wave-uniform: every load in flight together
#pragma unroll
        for (int k = 0; k < RADIX_ITEMS; ++k) qv[k] = in[base + k * 64 + lane].q0;
    } else {
#pragma unroll
        for (int k = 0; k < RADIX_ITEMS; ++k) {
            const uint32_t i = base + k * 64 + lane;
            qv[k] = i < n ? in[i].q0 : REC_SENTINEL;
        }
    }
    // counts only (no ranks): one LDS atomic per record into the wave's own row
#pragma unroll
    for (int k = 0; k < RADIX_ITEMS; ++k) {
        const uint32_t i = base + k * 64 + lane;
        const bool valid = i < n && (!SPARSE || qv[k] != REC_SENTINEL);
        if (valid) atomicAdd(&cnt[w][dig(qv[k])], 1u);
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < D; d += RADIX_THREADS) {
        uint32_t t = 0;
#pragma unroll
        for (int ww = 0; ww < RADIX_NW; ++ww) t += cnt[ww][d];
        hist[(size_t)d * gridDim.x + cb] = t;
    }
}

// The same counts from the digit bytes the previous pass wrote next to its
// output (1 B per record instead of a 16-B record line).  A block counts PER
// consecutive radix chunks (logical block XCD-contiguous, so a histogram row's
// neighbouring chunks meet in one L2): thread t loads bytes [8t, 8t+8) of each
// of them -- every load in flight together -- into LDS counters [digit][chunk].  One
// chunk per block was 13 k blocks of 512 threads at SwissProt scale, ~51 us a
// pass for 54 MB of digits: dispatch, not bytes.
// WAVE_ROWS: every wave counts into its own row of 16-bit counters (two per
// word: a wave adds at most 64 x 8 to one (digit, chunk)), summed over the
// waves at the end -- the block-shared counters took ~9 conflict cycles per
// LDS instruction (SQ, r04y).
constexpr uint32_t HIST_U8_PER_MAX = 8;
template <bool WAVE_ROWS>
__global__ void __launch_bounds__(RADIX_THREADS)
k_radix_hist_u8(const uint8_t* __restrict__ dig, uint32_t n, int bits, uint32_t* __restrict__ hist, uint32_t G,
                uint32_t per, const unsigned long long* __restrict__ dn) {
    constexpr uint32_t ROW = HIST_U8_PER_MAX * RADIX_D / 2;  // words of one wave's packed row
    __shared__ uint32_t cnt[WAVE_ROWS ? RADIX_NW * ROW : HIST_U8_PER_MAX * RADIX_D];
    if (dn) n = (uint32_t)min((unsigned long long)n, *dn);
    const uint32_t D = 1u << bits;
    for (uint32_t i = threadIdx.x; i < (WAVE_ROWS ? RADIX_NW * ROW : per * D); i += RADIX_THREADS) cnt[i] = 0;
    static_assert(RADIX_ITEMS == 8, "one 8-B load per thread and chunk");
    const uint32_t c0 = xcd_contiguous_block() * per;
    uint2 v[HIST_U8_PER_MAX];
    uint32_t nv[HIST_U8_PER_MAX];  // digits of this thread below n, per chunk
#pragma unroll
    for (uint32_t j = 0; j < HIST_U8_PER_MAX; ++j) {
        v[j] = make_uint2(0u, 0u);
        nv[j] = 0;
        const uint32_t i0 = (c0 + j) * RADIX_CHUNK + threadIdx.x * RADIX_ITEMS;
        if (j < per && c0 + j < G) {
            if (i0 + RADIX_ITEMS <= n) {
                v[j] = *reinterpret_cast<const uint2*>(dig + i0);
                nv[j] = RADIX_ITEMS;
            } else if (i0 < n) {
                uint32_t b[2] = {0u, 0u};
                nv[j] = n - i0;
                for (uint32_t k = 0; k < nv[j]; ++k) b[k >> 2] |= (uint32_t)dig[i0 + k] << (8 * (k & 3));
                v[j] = make_uint2(b[0], b[1]);
            }
        }
    }
    __syncthreads();
    uint32_t* const row = cnt + (WAVE_ROWS ? (threadIdx.x >> 6) * ROW : 0u);
#pragma unroll
    for (uint32_t j = 0; j < HIST_U8_PER_MAX; ++j) {
#pragma unroll
        for (uint32_t k = 0; k < RADIX_ITEMS; ++k) {
            const uint32_t d = ((k < 4 ? v[j].x : v[j].y) >> (8 * (k & 3))) & 0xFFu;
            if (k < nv[j]) {
                if constexpr (WAVE_ROWS) {
                    const uint32_t x = d * per + j;
                    atomicAdd(&row[x >> 1], 1u << (16 * (x & 1)));
                } else {
                    atomicAdd(&cnt[d * per + j], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < per * D; i += RADIX_THREADS) {
        const uint32_t d = i / per, j = i - d * per;  // consecutive threads: one row's consecutive chunks
        uint32_t t;
        if constexpr (WAVE_ROWS) {
            t = 0;
#pragma unroll
            for (uint32_t ww = 0; ww < RADIX_NW; ++ww) t += (cnt[ww * ROW + (i >> 1)] >> (16 * (i & 1))) & 0xFFFFu;
        } else {
            t = cnt[i];
        }
        if (c0 + j < G) hist[(size_t)d * G + c0 + j] = t;
    }
}

// NARROW: only the second word q1 of each record (after xform) is written, as
// one u64 per record (the owner exchange of a sharded build: 8 B on the wire)
template <bool SPARSE, typename Digit, bool NARROW = false>
__global__ void __launch_bounds__(RADIX_THREADS)
k_radix_scatter(const Rec* __restrict__ in, void* __restrict__ out, uint32_t n, Digit dig, int bits,
                const uint32_t* __restrict__ offs, uint8_t* __restrict__ nd_out, int nshift, uint32_t nmask,
                const unsigned long long* __restrict__ dn) {
    static_assert(RADIX_D <= RADIX_THREADS, "one digit per thread");
    static_assert(RADIX_CHUNK <= 65535, "16-bit counts");
    __shared__ uint16_t cnt[RADIX_NW][RADIX_D];
    __shared__ uint4 stage[RADIX_CHUNK];  // the block's records in digit order
    __shared__ uint16_t sdig[RADIX_CHUNK];  // their digit | next pass's digit << 8 (computed once)
    __shared__ uint32_t gofs[RADIX_D];    // global position of digit d's first record - its local start
    __shared__ uint32_t s_tmp[RADIX_NW + 1];
    if (dn) n = (uint32_t)min((unsigned long long)n, *dn);
    const uint32_t D = 1u << bits;
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    for (uint32_t d = lane; d < D; d += 64) cnt[w][d] = 0;
    wave_sync();
    const uint32_t cb = radix_chunk();
    const uint32_t base = cb * RADIX_CHUNK + w * (RADIX_ITEMS * 64);
    const uint4* __restrict__ in4 = reinterpret_cast<const uint4*>(in);
    uint4 rv[RADIX_ITEMS];
    if (base + RADIX_ITEMS * 64 <= n) {  // wave-uniform: every load in flight together
#pragma unroll
        for (int k = 0; k < RADIX_ITEMS; ++k) rv[k] = in4[base + k * 64 + lane];
    } else {  // the last records (a load per branch: one round trip each)
#pragma unroll
        for (int k = 0; k < RADIX_ITEMS; ++k) {
            const uint32_t i = base + k * 64 + lane;
            rv[k] = i < n ? in4[i] : make_uint4(0, 0, 0, 0);
        }
    }
    // this block's global digit offsets, in flight with the records (one per thread)
    const uint32_t goff = threadIdx.x < D ? offs[(size_t)threadIdx.x * gridDim.x + cb] : 0u;
    // rank of every record among the wave's earlier records of its digit
    uint32_t dg[RADIX_ITEMS], pos[RADIX_ITEMS];
    uint32_t vmask = 0;
#pragma unroll
    for (int k = 0; k < RADIX_ITEMS; ++k) {
        const uint32_t i = base + k * 64 + lane;
        const bool valid = i < n && (!SPARSE || (rv[k].x & rv[k].y) != 0xFFFFFFFFu);
        vmask |= (uint32_t)valid << k;
        const uint32_t dd = dig.both(u4_q0(rv[k]), nshift, nmask);
        const uint32_t d = dd & 0xFFu;
        const uint64_t peers = digit_peers(d, valid, bits);
        const uint32_t rank = (uint32_t)__popcll(peers & lanemask_lt());
        const uint32_t before = cnt[w][d];
        wave_sync();
        if (valid && rank == 0) cnt[w][d] = (uint16_t)(before + (uint32_t)__popcll(peers));
        wave_sync();
        dg[k] = dd;
        pos[k] = before + rank;
    }
    __syncthreads();
    // per digit (one per thread): block-local start (scan over digits), the
    // waves in order inside it, and the global offset of this block's run
    const uint32_t d = threadIdx.x;
    uint32_t tot = 0;
    if (d < D) {
#pragma unroll
        for (int ww = 0; ww < RADIX_NW; ++ww) tot += cnt[ww][d];
    }
    uint32_t nvalid;
    const uint32_t lstart = block_excl_scan<RADIX_THREADS, uint32_t>(tot, s_tmp, nvalid);
    if (d < D) {
        uint32_t acc = lstart;
#pragma unroll
        for (int ww = 0; ww < RADIX_NW; ++ww) {
            const uint32_t t = cnt[ww][d];
            cnt[ww][d] = (uint16_t)acc;
            acc += t;
        }
        gofs[d] = goff - lstart;
    }
    __syncthreads();
    // exchange through LDS, then write digit runs with consecutive lanes on
    // consecutive addresses
#pragma unroll
    for (int k = 0; k < RADIX_ITEMS; ++k) {
        if (vmask & (1u << k)) {
            const uint32_t at = cnt[w][dg[k] & 0xFFu] + pos[k];
            stage[at] = rv[k];
            sdig[at] = (uint16_t)dg[k];
        }
    }
    __syncthreads();
    uint4* __restrict__ out4 = reinterpret_cast<uint4*>(out);
    unsigned long long* __restrict__ out8 = reinterpret_cast<unsigned long long*>(out);
    for (uint32_t t = threadIdx.x; t < nvalid; t += RADIX_THREADS) {
        uint4 r = stage[t];
        const uint32_t dd = sdig[t];
        const uint32_t at = gofs[dd & 0xFFu] + t;
        if (nd_out) nd_out[at] = (uint8_t)(dd >> 8);
        dig.xform(r);
        if (NARROW) out8[at] = u4_q1(r);
        else out4[at] = r;
    }
}

template <typename Digit>
static hipError_t radix_hist(const Rec* d_in, uint32_t n, const Digit& dig, int bits, bool sparse, uint32_t* d_hist,
                             hipStream_t s, const unsigned long long* d_n = nullptr) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (n + RADIX_CHUNK - 1) / RADIX_CHUNK;
    if (sparse)
        DBI_LAUNCH((k_radix_hist<true, Digit>), dim3(g), dim3(RADIX_THREADS), 0, s, d_in, n, dig, bits, d_hist, d_n);
    else
        DBI_LAUNCH((k_radix_hist<false, Digit>), dim3(g), dim3(RADIX_THREADS), 0, s, d_in, n, dig, bits, d_hist, d_n);
    return hipGetLastError();
}

template <typename Digit>
static hipError_t radix_scatter(const Rec* d_in, Rec* d_out, uint32_t n, const Digit& dig, int bits, bool sparse,
                                const uint32_t* d_hist, hipStream_t s, uint8_t* nd_out = nullptr, int nshift = 0,
                                int nbits = 0, const unsigned long long* d_n = nullptr) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (n + RADIX_CHUNK - 1) / RADIX_CHUNK;
    const uint32_t nmask = (1u << nbits) - 1;
    if (sparse)
        DBI_LAUNCH((k_radix_scatter<true, Digit>), dim3(g), dim3(RADIX_THREADS), 0, s, d_in, d_out, n, dig, bits,
                   d_hist, nd_out, nshift, nmask, d_n);
    else
        DBI_LAUNCH((k_radix_scatter<false, Digit>), dim3(g), dim3(RADIX_THREADS), 0, s, d_in, d_out, n, dig, bits,
                   d_hist, nd_out, nshift, nmask, d_n);
    return hipGetLastError();
}

hipError_t launch_radix_hist(const Rec* d_in, uint32_t n, const BinMap& bm, int shift, int bits, bool sparse,
                             uint32_t* d_hist, hipStream_t s, const unsigned long long* d_n) {
    return radix_hist(d_in, n, BinDigit{bm, shift, (1u << bits) - 1}, bits, sparse, d_hist, s, d_n);
}

hipError_t launch_radix_hist_u8(const uint8_t* d_dig, uint32_t n, int bits, uint32_t* d_hist, hipStream_t s,
                                const unsigned long long* d_n) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (n + RADIX_CHUNK - 1) / RADIX_CHUNK;
    const uint32_t per = std::min<uint32_t>(HIST_U8_PER_MAX, std::max<uint32_t>(1u, g / 2048u));
    DBI_LAUNCH(k_radix_hist_u8<true>, dim3((g + per - 1) / per), dim3(RADIX_THREADS), 0, s, d_dig, n, bits, d_hist,
               g, per, d_n);
    return hipGetLastError();
}

hipError_t launch_radix_scatter(const Rec* d_in, Rec* d_out, uint32_t n, const BinMap& bm, int shift, int bits,
                                bool sparse, const uint32_t* d_hist, hipStream_t s, uint8_t* d_next_dig,
                                int next_shift, int next_bits, const unsigned long long* d_n) {
    return radix_scatter(d_in, d_out, n, BinDigit{bm, shift, (1u << bits) - 1}, bits, sparse, d_hist, s, d_next_dig,
                         next_shift, next_bits, d_n);
}

// owner partition of a sharded build: the same stable pass with digit = owner
// shard of the record's mass key, and the shard's first global protein id
// folded into every record on the way out
hipError_t launch_owner_hist(const Rec* d_in, uint32_t n, const OwnerMap& om, bool sparse, uint32_t* d_hist,
                             hipStream_t s, const unsigned long long* d_n) {
    return radix_hist(d_in, n, OwnerDigit{om}, owner_bits(om.nshards), sparse, d_hist, s, d_n);
}

hipError_t launch_owner_scatter(const Rec* d_in, uint64_t* d_out, uint32_t n, const OwnerMap& om, bool sparse,
                                const uint32_t* d_hist, hipStream_t s, const unsigned long long* d_n) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (n + RADIX_CHUNK - 1) / RADIX_CHUNK;
    const OwnerDigit dig{om};
    const int bits = owner_bits(om.nshards);
    if (sparse)
        DBI_LAUNCH((k_radix_scatter<true, OwnerDigit, true>), dim3(g), dim3(RADIX_THREADS), 0, s, d_in, (void*)d_out,
                   n, dig, bits, d_hist, (uint8_t*)nullptr, 0, 0u, d_n);
    else
        DBI_LAUNCH((k_radix_scatter<false, OwnerDigit, true>), dim3(g), dim3(RADIX_THREADS), 0, s, d_in, (void*)d_out,
                   n, dig, bits, d_hist, (uint8_t*)nullptr, 0, 0u, d_n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 4'. depth bins (warm lean builds): the map, the pass-2 plan, the pass over
// the low digit, the chunk bounds.  See PartOut / part_tile.
// ---------------------------------------------------------------------------
// ns uniques of the previous index, evenly spaced (so in mass order): each
// one's sub-bin and occurrence weight (capped at 4096: the weights' scan stays
// in 32 bits; a heavier spike is heavy either way)
__global__ void k_depth_sample(const double* __restrict__ umass, const uint32_t* __restrict__ occ_off, uint64_t nu,
                               uint32_t ns, BinMap sub, uint32_t* __restrict__ ss, uint32_t* __restrict__ sw) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const uint64_t j = (uint64_t)i * nu / ns;
    const uint32_t w = occ_off[j + 1] - occ_off[j];
    ss[i] = bin_of(umass[j], sub);
    sw[i] = w <= (1u << 24) ? min(w, 4096u) : 0u;  // (a stale index: never a wild weight)
}

hipError_t launch_depth_sample(const double* d_umass, const uint32_t* d_occ_off, uint64_t n_unique, uint32_t ns,
                               const BinMap& sub, uint32_t* d_ss, uint32_t* d_sw, hipStream_t s) {
    if (n_unique < ns) return hipErrorInvalidValue;
    if (ns == 0) return hipSuccess;
    DBI_LAUNCH(k_depth_sample, dim3((ns + 255) / 256), dim3(256), 0, s, d_umass, d_occ_off, n_unique, ns, sub, d_ss,
               d_sw);
    return hipGetLastError();
}

// Bin starts.  Sample i starts a bin at its sub-bin when its weight quantile
// pre * nq / total differs from its predecessor's (equal depth); a heavy
// sub-bin -- sampled weight above one mean bin, an isobaric cluster or a
// spike -- gets a bin of its own (starts at it and after it), so a bin never
// holds a heavy sub-bin plus its quantile's share (SwissProt: 787 -> ~420
// depth bins above the 1 984-record chunk capacity, tools/depth_sim.py).
// nq leaves room for the map's heavy sub-bins (2 starts each), counted by a
// first pass of the same kernel (COUNT; the handle's first map had no count
// to go by when the room came from the previous map's, and its extra starts
// piled the top quantiles into the last bin: a region overflow at SwissProt
// scale); the bins stay <= nbins, more heavies than that only merge the top.
template <bool COUNT>
__global__ void k_depth_mark(const uint32_t* __restrict__ ss, const uint32_t* __restrict__ pre, uint32_t ns,
                             uint32_t nbins, uint32_t nsub, uint4* __restrict__ map, Counters* __restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const unsigned long long tot = ctr->depth_w;
    if (tot == 0) return;
    const uint32_t s = ss[i];
    auto start = [&](uint32_t b) {
        if (b > 0 && b < nsub) atomicOr(reinterpret_cast<unsigned long long*>(&map[b >> 6]), 1ull << (b & 63u));
    };
    if (!COUNT) {
        const uint32_t hp = ctr->depth_hc;
        const uint64_t nq = 4ull * hp <= nbins ? nbins - 2ull * hp : nbins / 2u;
        if (i > 0 && (uint64_t)pre[i] * nq / tot != (uint64_t)pre[i - 1] * nq / tot) start(s);
    }
    if (i > 0 && ss[i - 1] == s) return;
    // the first sample of its sub-bin: the run's end by galloping (samples are
    // in mass order; most runs are one sample), its weight
    uint32_t lo = i + 1, step = 1;  // ss[lo - 1] == s
    while (lo < ns && ss[lo] == s) {
        const uint32_t hi = min(ns, lo + step);
        if (hi == lo + step && ss[hi - 1] == s) {
            lo = hi;
            step *= 2;
            continue;
        }
        uint32_t a = lo, b = hi - 1;  // ss[a] == s, the end in (a, b]
        while (a + 1 < b) {
            const uint32_t m = (a + b) >> 1;
            if (ss[m] == s) a = m; else b = m;
        }
        lo = ss[b] == s ? b + 1 : b;
        break;
    }
    const uint64_t w = (lo < ns ? (uint64_t)pre[lo] : tot) - pre[i];
    if (w * nbins > tot) {
        if (COUNT) {
            atomicAdd(&ctr->depth_hc, 1u);
        } else {
            start(s);
            start(s + 1);
            atomicAdd(&ctr->depth_h, 1u);
        }
    }
}

// map[w].z = bin starts in the words before w: one thread per word, NT words
// a block; a block's offset is the popcount of every word before it (each
// thread sums a strided share, issued together: L2-resident, one launch in
// place of a multi-launch scan).  *heavy = this map's heavy count.
template <int NT>
__global__ void __launch_bounds__(NT) k_depth_base(uint4* __restrict__ map, uint32_t G, uint32_t* __restrict__ heavy,
                                                   const Counters* __restrict__ ctr) {
    __shared__ uint32_t s_tmp[NT / 64 + 1];
    const uint32_t w = blockIdx.x * NT + threadIdx.x;
    uint32_t before = 0;
    for (uint32_t i = threadIdx.x; i < blockIdx.x * NT; i += NT) {
        const uint4 e = map[i];
        before += (uint32_t)__popc(e.x) + (uint32_t)__popc(e.y);
    }
    const uint4 e = w < G ? map[w] : make_uint4(0, 0, 0, 0);
    const uint32_t c = (uint32_t)__popc(e.x) + (uint32_t)__popc(e.y);
    uint32_t boff;
    block_excl_scan<NT, uint32_t>(before, s_tmp, boff);  // (the block's sum of `before`: its offset)
    uint32_t tot;
    const uint32_t run = block_excl_scan<NT, uint32_t>(c, s_tmp, tot);
    if (w < G) map[w].z = boff + run;
    if (w == 0) *heavy = ctr->depth_h;
}

hipError_t launch_depth_map(const uint32_t* d_ss, const uint32_t* d_pre, uint32_t ns, uint32_t nbins, uint32_t nsub,
                            uint4* d_map, uint32_t* d_heavy, Counters* d_ctr, hipStream_t s) {
    if (nbins == 0 || nbins > 65536u || nsub < 64 || (nsub & (nsub - 1))) return hipErrorInvalidValue;
    if (ns)  // (no sample: one bin; the regions overflow and the radix tail redoes the build)
        DBI_LAUNCH(k_depth_mark<true>, dim3((ns + 255) / 256), dim3(256), 0, s, d_ss, d_pre, ns, nbins, nsub, d_map,
                   d_ctr);
    if (ns)
        DBI_LAUNCH(k_depth_mark<false>, dim3((ns + 255) / 256), dim3(256), 0, s, d_ss, d_pre, ns, nbins, nsub, d_map,
                   d_ctr);
    const uint32_t G = nsub / 64;
    DBI_LAUNCH(k_depth_base<1024>, dim3((G + 1023) / 1024), dim3(1024), 0, s, d_map, G, d_heavy, d_ctr);
    return hipGetLastError();
}

// One block: region counts -> pass-2 chunks (PART_CHUNK-record pieces of each
// region, digit-major, XCD, piece), the first chunk and chunk count of every
// high digit, ctr->part_chunks; the records to sort (ctr->tail_n), or 0 when
// the digest's slots or a region overflowed.
__global__ void __launch_bounds__(256)
k_part_plan(const uint32_t* __restrict__ cur, uint32_t cap, uint32_t b1, uint64_t slot_cap,
            uint32_t* __restrict__ desc, uint32_t* __restrict__ d1c, Counters* __restrict__ ctr) {
    __shared__ uint32_t s_tmp[256 / 64 + 1];
    const uint32_t d = threadIdx.x, D1 = 1u << b1;
    // every cursor's adds accounted for: the regions hold exactly the kept records
    uint32_t placed = 0;
    if (d < D1) {
#pragma unroll
        for (uint32_t x = 0; x < DEPTH_XCDS; ++x) placed += cur[x * 256u + d];
    }
    uint32_t all_placed;
    block_excl_scan<256, uint32_t>(placed, s_tmp, all_placed);
    // the records must fit the tail's buffers too: a tile staged in LDS
    // reserves no slots, so n_slots alone no longer bounds n_kept (a grown
    // proteome: nothing downstream runs, the host grows them and redoes it)
    const bool fits = ctr->n_slots <= slot_cap && ctr->n_kept <= slot_cap;
    const bool ok = fits && !(ctr->err & ERR_PART) && all_placed == ctr->n_kept;
    if (d == 0 && !(ctr->err & ERR_PART) && fits && all_placed != ctr->n_kept)
        atomicOr(&ctr->err, ERR_PART);  // (lost cursor adds: redone by the radix tail)
    uint32_t nch = 0;
    if (ok && d < D1) {
#pragma unroll
        for (uint32_t x = 0; x < DEPTH_XCDS; ++x) nch += (cur[x * 256u + d] + PART_CHUNK - 1) / PART_CHUNK;
    }
    uint32_t total;
    uint32_t first = block_excl_scan<256, uint32_t>(nch, s_tmp, total);
    if (d < D1) {
        d1c[d] = first;
        d1c[D1 + d] = nch;
    }
    if (ok && d < D1) {
        for (uint32_t x = 0; x < DEPTH_XCDS; ++x) {
            const uint32_t r = d * DEPTH_XCDS + x, k1 = (cur[x * 256u + d] + PART_CHUNK - 1) / PART_CHUNK;
            for (uint32_t k = 0; k < k1; ++k) desc[first++] = r << 16 | k;
        }
    }
    if (d == 0) {
        ctr->part_chunks = total;
        ctr->tail_n = ok ? ctr->n_kept : 0ull;
        ctr->tail_in = ok ? ctr->n_kept : 0ull;
    }
}

hipError_t launch_part_plan(const uint32_t* d_cur, uint32_t cap, uint32_t b1, uint64_t slot_cap, uint32_t* d_desc,
                            uint32_t* d_d1c, Counters* d_ctr, hipStream_t s) {
    if (b1 < 1 || b1 > 8 || cap / PART_CHUNK >= 65536u) return hipErrorInvalidValue;
    DBI_LAUNCH(k_part_plan, dim3(1), dim3(256), 0, s, d_cur, cap, b1, slot_cap, d_desc, d_d1c, d_ctr);
    return hipGetLastError();
}

// pass-2 chunk c: its records [*lo, *lo + *n) of the region buffer, its high
// digit's first chunk and chunk count
struct PartChunk {
    uint32_t lo, n, first, nch;
};
__device__ __forceinline__ PartChunk part_chunk(uint32_t c, const uint32_t* __restrict__ cur, uint32_t cap,
                                                const uint32_t* __restrict__ desc,
                                                const uint32_t* __restrict__ d1c, uint32_t b1) {
    const uint32_t r = desc[c] >> 16, k = desc[c] & 0xFFFFu, d1 = r / DEPTH_XCDS;
    PartChunk pc;
    pc.lo = r * cap + k * PART_CHUNK;
    pc.n = min(PART_CHUNK, cur[(r % DEPTH_XCDS) * 256u + d1] - k * PART_CHUNK);
    pc.first = d1c[d1];
    pc.nch = d1c[(1u << b1) + d1];
    return pc;
}

__device__ __forceinline__ uint32_t part_hidx(const PartChunk& pc, uint32_t c, uint32_t d2, uint32_t b2) {
    return (pc.first << b2) + d2 * pc.nch + (c - pc.first);
}

// the pass-2 digits (bytes) of one chunk counted in per-wave LDS rows.  LSD:
// the histogram is digit-major over every chunk of the grid (the chunks past
// ctr->part_chunks count nothing), so the scan orders records by (d2, d1)
template <bool LSD>
__global__ void __launch_bounds__(RADIX_THREADS)
k_part_hist(const uint8_t* __restrict__ dig, const uint32_t* __restrict__ cur, uint32_t cap,
            const uint32_t* __restrict__ desc, const uint32_t* __restrict__ d1c, uint32_t b1, uint32_t b2,
            uint32_t* __restrict__ hist, const Counters* __restrict__ ctr) {
    __shared__ uint32_t cnt[RADIX_NW][RADIX_D];
    const uint32_t c = xcd_contiguous_block();
    const uint32_t w = threadIdx.x >> 6, D2 = 1u << b2;
    if (c >= ctr->part_chunks) {
        if (LSD)
            for (uint32_t d = threadIdx.x; d < D2; d += RADIX_THREADS) hist[(size_t)d * gridDim.x + c] = 0u;
        return;
    }
    for (uint32_t d = lane_id(); d < D2; d += 64) cnt[w][d] = 0;
    const PartChunk pc = part_chunk(c, cur, cap, desc, d1c, b1);
    static_assert(PART_CHUNK == RADIX_THREADS * 8, "one 8-B load per thread");
    const uint32_t i0 = threadIdx.x * 8;
    uint2 v = make_uint2(0u, 0u);
    if (i0 < pc.n) v = *reinterpret_cast<const uint2*>(dig + pc.lo + i0);  // (lo and cap: multiples of 64)
    wave_sync();
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        if (i0 + k < pc.n) atomicAdd(&cnt[w][((k < 4 ? v.x : v.y) >> (8 * (k & 3))) & 0xFFu], 1u);
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < D2; d += RADIX_THREADS) {
        uint32_t t = 0;
#pragma unroll
        for (uint32_t ww = 0; ww < (uint32_t)RADIX_NW; ++ww) t += cnt[ww][d];
        hist[LSD ? (size_t)d * gridDim.x + c : part_hidx(pc, c, d, b2)] = t;
    }
}

hipError_t launch_part_hist(const uint8_t* d_dig, const uint32_t* d_cur, uint32_t cap, const uint32_t* d_desc,
                            const uint32_t* d_d1c, uint32_t b1, uint32_t b2, uint32_t max_chunks, uint32_t* d_hist,
                            const Counters* d_ctr, hipStream_t s, bool lsd) {
    if (max_chunks == 0) return hipSuccess;
    if (b2 < 1 || b2 > (uint32_t)RADIX_BITS) return hipErrorInvalidValue;
    if (lsd)
        DBI_LAUNCH(k_part_hist<true>, dim3(max_chunks), dim3(RADIX_THREADS), 0, s, d_dig, d_cur, cap, d_desc, d_d1c,
                   b1, b2, d_hist, d_ctr);
    else
        DBI_LAUNCH(k_part_hist<false>, dim3(max_chunks), dim3(RADIX_THREADS), 0, s, d_dig, d_cur, cap, d_desc, d_d1c,
                   b1, b2, d_hist, d_ctr);
    return hipGetLastError();
}

// The pass over the low digit: a chunk's records ranked per digit in input
// order (wave ballots, as k_radix_scatter), exchanged through LDS and written
// as digit runs to their (high digit, low digit) = bin place.  LSD: the
// second pass of linear bins (order (d2, d1)), each record's next-pass digit
// written beside it (ndig), as k_radix_scatter does.
template <bool LSD>
__global__ void __launch_bounds__(RADIX_THREADS)
k_part_scatter(const Rec* __restrict__ recs, const uint8_t* __restrict__ dig, const uint32_t* __restrict__ cur,
               uint32_t cap, const uint32_t* __restrict__ desc, const uint32_t* __restrict__ d1c, uint32_t b1,
               uint32_t b2, const uint32_t* __restrict__ offs, Rec* __restrict__ out,
               const Counters* __restrict__ ctr, uint8_t* __restrict__ ndig, BinMap bm, uint32_t nshift,
               uint32_t nbits) {
    __shared__ uint16_t cnt[RADIX_NW][RADIX_D];
    __shared__ uint4 stage[RADIX_CHUNK];
    __shared__ uint8_t sdig[RADIX_CHUNK];
    __shared__ uint32_t gofs[RADIX_D];
    __shared__ uint32_t s_tmp[RADIX_NW + 1];
    const uint32_t c = xcd_contiguous_block();
    if (c >= ctr->part_chunks) return;
    const uint32_t D2 = 1u << b2;
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    for (uint32_t d = lane; d < D2; d += 64) cnt[w][d] = 0;
    wave_sync();
    const PartChunk pc = part_chunk(c, cur, cap, desc, d1c, b1);
    const uint32_t base = w * (RADIX_ITEMS * 64);  // this wave's records, chunk-relative
    const uint4* __restrict__ in4 = reinterpret_cast<const uint4*>(recs + pc.lo);
    uint4 rv[RADIX_ITEMS];
    uint32_t dd[RADIX_ITEMS];
    if (base + RADIX_ITEMS * 64 <= pc.n) {  // wave-uniform: every load in flight together
#pragma unroll
        for (int k = 0; k < RADIX_ITEMS; ++k) rv[k] = in4[base + k * 64 + lane];
#pragma unroll
        for (int k = 0; k < RADIX_ITEMS; ++k) dd[k] = dig[pc.lo + base + k * 64 + lane];
    } else {
#pragma unroll
        for (int k = 0; k < RADIX_ITEMS; ++k) {
            const uint32_t i = base + k * 64 + lane;
            rv[k] = i < pc.n ? in4[i] : make_uint4(0, 0, 0, 0);
            dd[k] = i < pc.n ? (uint32_t)dig[pc.lo + i] : 0u;
        }
    }
    const uint32_t goff =
        threadIdx.x < D2 ? offs[LSD ? (size_t)threadIdx.x * gridDim.x + c : part_hidx(pc, c, threadIdx.x, b2)] : 0u;
    uint32_t pos[RADIX_ITEMS];
    uint32_t vmask = 0;
#pragma unroll
    for (int k = 0; k < RADIX_ITEMS; ++k) {
        const bool valid = base + k * 64 + lane < pc.n;
        vmask |= (uint32_t)valid << k;
        const uint32_t d = dd[k];
        const uint64_t peers = digit_peers(d, valid, (int)b2);
        const uint32_t rank = (uint32_t)__popcll(peers & lanemask_lt());
        const uint32_t before = cnt[w][d];
        wave_sync();
        if (valid && rank == 0) cnt[w][d] = (uint16_t)(before + (uint32_t)__popcll(peers));
        wave_sync();
        pos[k] = before + rank;
    }
    __syncthreads();
    const uint32_t d = threadIdx.x;
    uint32_t tot = 0;
    if (d < D2) {
#pragma unroll
        for (int ww = 0; ww < RADIX_NW; ++ww) tot += cnt[ww][d];
    }
    uint32_t nvalid;
    const uint32_t lstart = block_excl_scan<RADIX_THREADS, uint32_t>(tot, s_tmp, nvalid);
    if (d < D2) {
        uint32_t acc = lstart;
#pragma unroll
        for (int ww = 0; ww < RADIX_NW; ++ww) {
            const uint32_t t = cnt[ww][d];
            cnt[ww][d] = (uint16_t)acc;
            acc += t;
        }
        gofs[d] = goff - lstart;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RADIX_ITEMS; ++k) {
        if (vmask & (1u << k)) {
            const uint32_t at = cnt[w][dd[k]] + pos[k];
            stage[at] = rv[k];
            sdig[at] = (uint8_t)dd[k];
        }
    }
    __syncthreads();
    uint4* __restrict__ out4 = reinterpret_cast<uint4*>(out);
    for (uint32_t t = threadIdx.x; t < nvalid; t += RADIX_THREADS) {
        const uint32_t at = gofs[sdig[t]] + t;
        out4[at] = stage[t];
        if (LSD && ndig) ndig[at] = (uint8_t)((bin_of(u4_mass(stage[t]), bm) >> nshift) & ((1u << nbits) - 1u));
    }
}

hipError_t launch_part_scatter(const Rec* d_recs, const uint8_t* d_dig, const uint32_t* d_cur, uint32_t cap,
                               const uint32_t* d_desc, const uint32_t* d_d1c, uint32_t b1, uint32_t b2,
                               uint32_t max_chunks, const uint32_t* d_offs, Rec* d_out, const Counters* d_ctr,
                               hipStream_t s, bool lsd, uint8_t* d_ndig, BinMap bm, uint32_t nshift, uint32_t nbits) {
    if (max_chunks == 0) return hipSuccess;
    if (b2 < 1 || b2 > (uint32_t)RADIX_BITS || (d_ndig && (!lsd || nbits < 1 || nbits > 8))) return hipErrorInvalidValue;
    if (lsd)
        DBI_LAUNCH(k_part_scatter<true>, dim3(max_chunks), dim3(RADIX_THREADS), 0, s, d_recs, d_dig, d_cur, cap,
                   d_desc, d_d1c, b1, b2, d_offs, d_out, d_ctr, d_ndig, bm, nshift, nbits);
    else
        DBI_LAUNCH(k_part_scatter<false>, dim3(max_chunks), dim3(RADIX_THREADS), 0, s, d_recs, d_dig, d_cur, cap,
                   d_desc, d_d1c, b1, b2, d_offs, d_out, d_ctr, d_ndig, bm, nshift, nbits);
    return hipGetLastError();
}

// bin b = (d1, d2) starts at the pass-2 offset of its first chunk's run
// (an empty high digit: where the next one starts); bstart[nbins] = records
__global__ void k_depth_starts(const uint32_t* __restrict__ offs, const uint32_t* __restrict__ d1c, uint32_t b1,
                               uint32_t b2, uint32_t* __restrict__ bstart, const Counters* __restrict__ ctr) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x, NB = 1u << (b1 + b2);
    if (b > NB) return;
    const uint32_t n = (uint32_t)ctr->tail_n;
    if (b == NB || n == 0) {
        bstart[b] = b == NB ? n : 0u;
        return;
    }
    const uint32_t d1 = b >> b2, d2 = b & ((1u << b2) - 1u);
    const uint32_t pos = (d1c[d1] << b2) + d2 * d1c[(1u << b1) + d1];
    bstart[b] = pos < (ctr->part_chunks << b2) ? offs[pos] : n;
}

// chunk pairs over the bins (k_chunk_bounds' layout): chunk 2c = the bins
// starting in [c*T, (c+1)*T), its last bin split off as chunk 2c+1 when the
// two together exceed CHUNK_CAP (a bin above it is a big chunk of its own)
// big_list (optional): the chunks above CHUNK_CAP listed here, so that the
// big tier can run beside the chunk sort (which then skips them)
__global__ void k_depth_chunks(const uint32_t* __restrict__ bstart, uint32_t nb, uint32_t T, uint32_t nchunks,
                               uint32_t* __restrict__ chunk_lo, Counters* __restrict__ ctr,
                               uint32_t* __restrict__ split_list, uint32_t* __restrict__ big_list) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nchunks) return;
    const uint32_t n = (uint32_t)ctr->tail_n;
    auto first_ge = [&](uint32_t x) {  // first b in [0, nb] with bstart[b] >= x (bstart[nb] = n >= x)
        uint32_t lo = 0, hi = nb;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (bstart[mid] >= x) hi = mid; else lo = mid + 1;
        }
        return lo;
    };
    const uint32_t x = c == nchunks ? n : (uint32_t)min((uint64_t)c * T, (uint64_t)n);
    const uint32_t s0 = bstart[first_ge(x)];
    chunk_lo[2 * c] = s0;
    if (c == nchunks) return;
    const uint32_t j1 = first_ge((uint32_t)min((uint64_t)(c + 1) * T, (uint64_t)n));
    const uint32_t s1 = bstart[j1];
    uint32_t split = s1;
    if (s1 - s0 > (uint32_t)CHUNK_CAP && j1 > 0 && bstart[j1 - 1] > s0) split = bstart[j1 - 1];
    chunk_lo[2 * c + 1] = split;
    if (split != s1) split_list[atomicAdd(&ctr->n_split, 1u)] = c;  // (k_chunk_sort runs these first)
    if (big_list) {
        if (split - s0 > (uint32_t)CHUNK_CAP) big_list[atomicAdd(&ctr->n_big, 1u)] = 2 * c;
        if (s1 - split > (uint32_t)CHUNK_CAP) big_list[atomicAdd(&ctr->n_big, 1u)] = 2 * c + 1;
    }
}

hipError_t launch_depth_bounds(const uint32_t* d_offs, const uint32_t* d_d1c, uint32_t b1, uint32_t b2,
                               uint32_t* d_bstart, uint32_t T, uint32_t nchunks, uint32_t* d_chunk_lo,
                               Counters* d_ctr, hipStream_t s, uint32_t* d_split_list, uint32_t* d_big_list) {
    const uint32_t nb = 1u << (b1 + b2);
    DBI_LAUNCH(k_depth_starts, dim3((nb + 1 + 255) / 256), dim3(256), 0, s, d_offs, d_d1c, b1, b2, d_bstart, d_ctr);
    DBI_LAUNCH(k_depth_chunks, dim3((nchunks + 1 + 255) / 256), dim3(256), 0, s, d_bstart, nb, T, nchunks, d_chunk_lo,
               d_ctr, d_split_list, d_big_list);
    return hipGetLastError();
}

// Owner side of the exchange: the (global protein, offset, length) word of
// each received occurrence -> its 16-B record, the mass and the tag
// recomputed from the residues exactly as the digest walk sums them
// (DBIndexer.java:265-308: m0, then one fp64 add per residue, left to right;
// -ffp-contract=off), so the record is bit-identical to the sender's.
constexpr uint32_t EXPAND_THREADS = 256;
__device__ __forceinline__ Rec expand_loc(uint64_t q1, const uint32_t* __restrict__ w32, uint32_t mis,
                                          const uint32_t* __restrict__ poff, const double* smass, double m0,
                                          uint32_t w) {
    const uint32_t len = q1_len(q1, w);
    // residues 16 at a time: the 5 dwords covering them loaded together
    // (clamped to the peptide's last dword) and realigned, as seq_equal_at
    const uint64_t ga = (uint64_t)poff[q1_pid(q1, w)] + q1_off(q1, w) + mis;
    const uint64_t last = (ga + len - 1) >> 2;
    double m = m0;
    uint32_t head = 0, tail = 0;
    for (uint32_t k0 = 0; k0 < len; k0 += 16) {
        const uint64_t ia = (ga + k0) >> 2;
        uint32_t wd[5];
#pragma unroll
        for (uint32_t j = 0; j < 5; ++j) wd[j] = w32[min(ia + j, last)];
        const uint32_t sa = (uint32_t)((ga + k0) & 3u);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t x = __builtin_amdgcn_alignbyte(wd[j + 1], wd[j], sa);
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                if (k0 + 4 * j + b < len) {  // sequential, left to right (DBIndexer.java:306-308)
                    const uint32_t c = (x >> (8 * b)) & 0xFFu;
                    m = m + smass[c];
                    if (k0 == 0 && j == 0) head |= c << (8 * b);
                    tail = (tail << 8) | c;
                }
            }
        }
    }
    const uint32_t tag = peptide_tag(head, tail, len);
    Rec r;
    r.q0 = rec_q0(m, tag);
    r.q1 = ((uint64_t)(tag & 0xFFu) << 56) | (q1 & 0x00FFFFFFFFFFFFFFull);  // pid | off | len as sent
    return r;
}

__global__ void __launch_bounds__(EXPAND_THREADS)
k_expand_locs(const unsigned long long* __restrict__ locs, uint64_t n, const uint8_t* __restrict__ res,
              const uint32_t* __restrict__ poff, const double* __restrict__ mass_tab, double m0, uint32_t w,
              Rec* __restrict__ out) {
    __shared__ double smass[256];
    for (uint32_t c = threadIdx.x; c < 256; c += EXPAND_THREADS) smass[c] = mass_tab[c];
    __syncthreads();
    // dword view of the residues (a buffer not 4-B aligned is read from the dword holding its first byte)
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(res) & 3u);
    const uint32_t* __restrict__ w32 = reinterpret_cast<const uint32_t*>(res - mis);
    for (uint64_t i = (uint64_t)blockIdx.x * EXPAND_THREADS + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * EXPAND_THREADS)
        out[i] = expand_loc(locs[i], w32, mis, poff, smass, m0, w);
}

hipError_t launch_expand_locs(const uint64_t* d_locs, uint64_t n, const uint8_t* d_res, const uint32_t* d_poff,
                              const double* d_mass_tab, double m0, uint32_t w, Rec* d_out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t g = (uint32_t)std::min<uint64_t>((n + EXPAND_THREADS - 1) / EXPAND_THREADS, 256u * 16u);
    DBI_LAUNCH(k_expand_locs, dim3(g), dim3(EXPAND_THREADS), 0, s, (const unsigned long long*)d_locs, n, d_res,
               d_poff, d_mass_tab, m0, w, d_out);
    return hipGetLastError();
}

// The same expansion with the owner merge's first radix pass histogram
// counted on the way: one block per radix chunk (RADIX_CHUNK records, the
// chunk of the scatter that follows: radix_chunk()), digit counts in LDS,
// hist[d * G + chunk] written by the block -- the tail skips that pass's
// histogram kernel, a read of every record's mass.
__global__ void __launch_bounds__(RADIX_THREADS)
k_expand_locs_hist(const unsigned long long* __restrict__ locs, uint32_t n, const uint8_t* __restrict__ res,
                   const uint32_t* __restrict__ poff, const double* __restrict__ mass_tab, double m0, uint32_t w,
                   Rec* __restrict__ out, BinMap bm, int bits, uint32_t* __restrict__ hist) {
    __shared__ double smass[256];
    __shared__ uint32_t cnt[RADIX_D];
    const uint32_t D = 1u << bits;
    for (uint32_t c = threadIdx.x; c < 256; c += RADIX_THREADS) smass[c] = mass_tab[c];
    for (uint32_t d = threadIdx.x; d < D; d += RADIX_THREADS) cnt[d] = 0;
    __syncthreads();
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(res) & 3u);
    const uint32_t* __restrict__ w32 = reinterpret_cast<const uint32_t*>(res - mis);
    const uint32_t cb = radix_chunk();
#pragma unroll 1
    for (uint32_t k = 0; k < RADIX_ITEMS; ++k) {
        const uint32_t i = cb * RADIX_CHUNK + k * RADIX_THREADS + threadIdx.x;
        if (i < n) {
            const Rec r = expand_loc(locs[i], w32, mis, poff, smass, m0, w);
            out[i] = r;
            atomicAdd(&cnt[bin_of(q0_mass(r.q0), bm) & (D - 1u)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < D; d += RADIX_THREADS) hist[(size_t)d * gridDim.x + cb] = cnt[d];
}

hipError_t launch_expand_locs_hist(const uint64_t* d_locs, uint32_t n, const uint8_t* d_res, const uint32_t* d_poff,
                                   const double* d_mass_tab, double m0, uint32_t w, Rec* d_out, const BinMap& bm,
                                   int bits, uint32_t* d_hist, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (bits < 1 || bits > RADIX_BITS) return hipErrorInvalidValue;
    const uint32_t g = (n + RADIX_CHUNK - 1) / RADIX_CHUNK;
    DBI_LAUNCH(k_expand_locs_hist, dim3(g), dim3(RADIX_THREADS), 0, s, (const unsigned long long*)d_locs, n, d_res,
               d_poff, d_mass_tab, m0, w, d_out, bm, bits, d_hist);
    return hipGetLastError();
}

// The owner merge on depth bins (round 6): the expansion
// partitions its records by the depth bin's high digit into (digit, XCD)
// regions exactly as the lean digest's tiles do (part_place: LDS ranks, one
// region reservation per digit, digit runs written by consecutive lanes), so
// the owner's records take the single-device tail from there -- one pass over
// the low digit (bin_scatter), the chunk sort binning each chunk in LDS,
// finalize -- instead of the radix tail's passes.  One block per
// EXPAND_PART_R received words.
constexpr uint32_t EXPAND_PART_R = 1024;  // (2048: 38 KiB of LDS, 16 waves per CU -- the gathers' latency showed)
__global__ void __launch_bounds__(DIGEST_THREADS)
k_expand_locs_part(const unsigned long long* __restrict__ locs, uint32_t n, const uint8_t* __restrict__ res,
                   const uint32_t* __restrict__ poff, const double* __restrict__ mass_tab, double m0, uint32_t w,
                   PartOut po, Counters* __restrict__ ctr) {
    constexpr uint32_t KI = EXPAND_PART_R / DIGEST_THREADS;
    static_assert(DIGEST_THREADS == 256, "one mass-table entry and one digit counter per thread");
    __shared__ double smass[256];
    __shared__ uint32_t s_cnt[256], s_run[256], s_tmp[DIGEST_THREADS / 64 + 1];
    __shared__ uint4 stage[EXPAND_PART_R];
    __shared__ uint16_t sdig[EXPAND_PART_R];
    const uint32_t tid = threadIdx.x;
    smass[tid] = mass_tab[tid];
    s_cnt[tid] = 0;
    __syncthreads();
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(res) & 3u);
    const uint32_t* __restrict__ w32 = reinterpret_cast<const uint32_t*>(res - mis);
    const uint32_t base = blockIdx.x * EXPAND_PART_R;
    const uint32_t nr = min(EXPAND_PART_R, n - base);
    // the expansion one record at a time (a residue gather loop per record:
    // not unrolled, few registers, many waves in flight), each into the stage
    // at its own index; then the records back into registers for part_place
    // (which restages them in digit order)
#pragma unroll 1
    for (uint32_t i = tid; i < nr; i += DIGEST_THREADS) {
        const Rec r = expand_loc(locs[base + i], w32, mis, poff, smass, m0, w);
        stage[i] = make_uint4((uint32_t)r.q0, (uint32_t)(r.q0 >> 32), (uint32_t)r.q1, (uint32_t)(r.q1 >> 32));
    }
    __syncthreads();
    uint4 rv[KI];
#pragma unroll
    for (uint32_t k = 0; k < KI; ++k) {
        const uint32_t i = k * DIGEST_THREADS + tid;
        rv[k] = i < nr ? stage[i] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);  // (past nr: part_place skips it)
    }
    __syncthreads();  // (part_place's restage overwrites the stage)
    part_place<KI>(po, rv, nr, s_cnt, s_run, s_tmp, stage, sdig, ctr);
}

hipError_t launch_expand_locs_part(const uint64_t* d_locs, uint32_t n, const uint8_t* d_res, const uint32_t* d_poff,
                                   const double* d_mass_tab, double m0, uint32_t w, const PartOut& po,
                                   Counters* d_ctr, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (po.lsd || po.b1 < 1 || po.b1 > 8 || po.dm.b2 < 1 || po.dm.b2 > 8) return hipErrorInvalidValue;
    const uint32_t g = (n + EXPAND_PART_R - 1) / EXPAND_PART_R;
    DBI_LAUNCH(k_expand_locs_part, dim3(g), dim3(DIGEST_THREADS), 0, s, (const unsigned long long*)d_locs, n, d_res,
               d_poff, d_mass_tab, m0, w, po, d_ctr);
    return hipGetLastError();
}

hipError_t launch_pair_hist(const Rec* d_in, uint32_t n, uint32_t nshards, uint32_t* d_hist, hipStream_t s) {
    return radix_hist(d_in, n, PairDigit{}, owner_bits(nshards), false, d_hist, s);
}

hipError_t launch_pair_scatter(const Rec* d_in, Rec* d_out, uint32_t n, uint32_t nshards, const uint32_t* d_hist,
                               hipStream_t s) {
    return radix_scatter(d_in, d_out, n, PairDigit{}, owner_bits(nshards), false, d_hist, s);
}

uint64_t radix_blocks(uint32_t n) { return (n + RADIX_CHUNK - 1) / RADIX_CHUNK; }

// ---------------------------------------------------------------------------
// 5. chunk sort + group by peptide string (IndexMerge.getMergedData :620-719)
// ---------------------------------------------------------------------------
// A chunk is a run of whole mass bins: chunk c = records [B(c*T), B((c+1)*T))
// with B(x) = start of the first bin starting at or after x.  Bins never
// straddle chunks, so sorting a chunk by mass equals sorting its bins, and
// chunk sizes stay near T whatever the mass-density skew.
// Same peptide string?  (The tie-break tag is 16 bits: equal (mass, tag) is
// not proof.)  16 residues per round: the 5 dwords covering them in each
// string are loaded together (addresses clamped to the string's last dword,
// so nothing past the string is read) and realigned with v_alignbyte — one
// memory round trip per 16 residues.  A residue buffer that is not 4-B aligned
// is read from the dword holding its first byte.
__device__ __forceinline__ bool seq_equal_at(const uint8_t* __restrict__ res, uint32_t g_a, uint32_t g_b,
                                             uint32_t len) {
    if (g_a == g_b) return true;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(res) & 3u);
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(res - mis);
    const uint64_t ga = (uint64_t)g_a + mis, gb = (uint64_t)g_b + mis;
    const uint64_t last_a = (ga + len - 1) >> 2, last_b = (gb + len - 1) >> 2;
    for (uint32_t k0 = 0; k0 < len; k0 += 16) {
        const uint64_t ia = (ga + k0) >> 2, ib = (gb + k0) >> 2;
        uint32_t wa[5], wb[5];
#pragma unroll
        for (uint32_t j = 0; j < 5; ++j) {
            wa[j] = w[min(ia + j, last_a)];
            wb[j] = w[min(ib + j, last_b)];
        }
        const uint32_t sa = (uint32_t)((ga + k0) & 3u), sb = (uint32_t)((gb + k0) & 3u);
        uint32_t diff = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t k = k0 + 4 * j;
            const uint32_t x = __builtin_amdgcn_alignbyte(wa[j + 1], wa[j], sa);
            const uint32_t y = __builtin_amdgcn_alignbyte(wb[j + 1], wb[j], sb);
            const uint32_t rem = k < len ? len - k : 0u;
            const uint32_t mask = rem >= 4 ? ~0u : ((1u << (8 * rem)) - 1u);
            diff |= (x ^ y) & mask;
        }
        if (diff) return false;
    }
    return true;
}

// Where a record's peptide sits in the residue buffer (poff[pid] + off), and its length.
struct RecLoc {
    const uint8_t* res;
    const uint32_t* poff;
    uint32_t w;
    __device__ __forceinline__ uint32_t gstart(uint64_t q1) const { return poff[q1_pid(q1, w)] + q1_off(q1, w); }
    __device__ __forceinline__ bool same(const Rec& a, const Rec& b) const {
        const uint32_t la = q1_len(a.q1, w);
        if (la != q1_len(b.q1, w)) return false;
        if ((a.q1 & 0x00FFFFFFFFFFFFFFull) == (b.q1 & 0x00FFFFFFFFFFFFFFull)) return true;
        return seq_equal_at(res, gstart(a.q1), gstart(b.q1), la);
    }
};

// record with the head flag in place of the tag (chunk sort -> finalize)
__device__ __forceinline__ Rec with_head(Rec r, bool head) {
    r.q0 = (r.q0 & ~0xFFull) | (head ? 1ull : 0ull);
    return r;
}

// Bitonic sort of (key, hsh, idx) triples, ascending; NT threads.
template <int NT>
__device__ void bitonic_sort3(unsigned long long* key, unsigned long long* hsh, uint32_t* k2, uint32_t P2) {
    for (uint32_t k = 2; k <= P2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < P2; i += NT) {
                const uint32_t ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = key[i], b = key[ixj];
                    const unsigned long long ha = hsh[i], hb = hsh[ixj];
                    const uint32_t ai = k2[i], bi = k2[ixj];
                    const bool gt = (a > b) || (a == b && (ha > hb || (ha == hb && ai > bi)));
                    const bool asc = (i & k) == 0;
                    if (asc ? gt : !gt) {
                        key[i] = b; key[ixj] = a;
                        hsh[i] = hb; hsh[ixj] = ha;
                        k2[i] = bi; k2[ixj] = ai;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// One chunk of n records above the LDS capacity, scratch in global memory.
// Sorted order = the record key (q0, q1) = (mass, tag, first appearance);
// equal (mass, tag) neighbours are string-verified; a 16-bit tag collision
// regroups its run by string, strings in first-appearance order.
// key/hsh/k2/k3 are P2-sized scratch; s_u32 >= NT/64+1 slots.
template <int NT>
__device__ uint32_t process_chunk(const Rec* __restrict__ in, Rec* __restrict__ out, uint32_t n, const RecLoc& rl,
                                  unsigned long long* key, unsigned long long* hsh, uint32_t* k2, uint32_t* k3,
                                  uint32_t* s_u32, unsigned long long* s_flag) {
    uint32_t P2 = 1;
    while (P2 < n) P2 <<= 1;
    for (uint32_t i = threadIdx.x; i < P2; i += NT) {
        if (i < n) {
            const Rec r = in[i];
            key[i] = r.q0;
            hsh[i] = r.q1;
        } else {
            key[i] = ~0ull;  // padding sorts last
            hsh[i] = ~0ull;
        }
        k2[i] = i;
    }
    if (threadIdx.x == 0) *s_flag = 0;
    __syncthreads();
    bitonic_sort3<NT>(key, hsh, k2, P2);
    auto same_tag = [&](uint32_t i) { return key[i] == key[i - 1] && (hsh[i] >> 56) == (hsh[i - 1] >> 56); };
    auto rec_at = [&](uint32_t i) { return Rec{key[i], hsh[i]}; };

    for (uint32_t i = threadIdx.x + 1; i < n; i += NT)
        if (same_tag(i) && !rl.same(rec_at(i), rec_at(i - 1))) atomicOr(s_flag, 1ull);
    __syncthreads();
    const bool regroup = *s_flag != 0;
    if (regroup) {
        // k3[i] = first position of the equal-(mass, tag) run containing i
        // (block max-scan of head positions; thread t owns [t*E, t*E+E))
        const uint32_t E = (n + NT - 1) / NT;
        const uint32_t lo = min(threadIdx.x * E, n), hi = min(lo + E, n);
        uint32_t last = 0;
        bool has = false;
        for (uint32_t i = lo; i < hi; ++i) {
            if (i == 0 || !same_tag(i)) { last = i; has = true; }
            k3[i] = last;
        }
        const int w = threadIdx.x >> 6;
        uint32_t inc = has ? last : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d, 64);
            if ((int)lane_id() >= d) inc = max(inc, o);
        }
        if (lane_id() == 63) s_u32[w] = inc;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t acc = 0;
            for (int i = 0; i < NT / 64; ++i) {
                const uint32_t t = s_u32[i];
                s_u32[i] = acc;
                acc = max(acc, t);
            }
        }
        __syncthreads();
        uint32_t excl = __shfl_up(inc, 1, 64);
        if (lane_id() == 0) excl = 0;
        excl = max(excl, s_u32[w]);
        for (uint32_t i = lo; i < hi; ++i) {
            if (i == 0 || !same_tag(i)) break;
            k3[i] = excl;
        }
        __syncthreads();
        // leader = first position of i's string in its run (positions in a run
        // follow first appearance; runs are disjoint ascending ranges, so the
        // leader position alone orders runs, then strings inside a run)
        for (uint32_t i = threadIdx.x; i < n; i += NT) {
            const uint32_t rs = k3[i];
            uint32_t leader = i;
            const Rec me = rec_at(i);
            for (uint32_t r = rs; r < i; ++r)
                if (rl.same(me, rec_at(r))) { leader = r; break; }
            k3[i] = leader;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += NT) key[i] = k3[i];
        __syncthreads();
        bitonic_sort3<NT>(key, hsh, k2, P2);  // -> (leader, occurrence); padding keeps ~0
    }

    // unique-peptide heads + write the chunk in final order
    uint32_t myheads = 0;
    for (uint32_t i = threadIdx.x; i < n; i += NT) {
        const bool head = (i == 0) || (regroup ? key[i] != key[i - 1] : !same_tag(i));
        out[i] = with_head(in[k2[i]], head);
        myheads += head;
    }
    return myheads;
}

// Chunk pairs over the bin-sorted records: chunk 2c = [start(c), split(c)),
// chunk 2c+1 = [split(c), start(c+1)), start(c) = the first bin start at or
// after c*T.  split(c) is the start of the bin that straddles (c+1)*T when
// that bin holds more than WAVE_SORT_LIMIT records and starts at or after c*T,
// else start(c+1): a big bin that crosses a boundary becomes a chunk of its
// own instead of carrying the chunk before it into the list kernels, and chunk
// 2c stays within T + WAVE_SORT_LIMIT records unless it is one bin.  Thread c
// finds the end of the bin straddling c*T (galloping, then binary search: a
// few loads for ordinary bins, log steps for mass spikes) and, only when one
// probe says the bin is big and another that it starts after (c-1)*T, its
// start by binary search inside that chunk width; it writes chunk_lo[2c] and
// chunk_lo[2c-1].  (One wave per boundary with 64 probes per step: 42 vs
// 35 us -- the probes' line traffic costs more than the shorter chains save.)
// chunk_lo has 2*nchunks + 1 entries.
__global__ void k_chunk_bounds(const Rec* __restrict__ recs, uint32_t n, BinMap bm, uint32_t T, uint32_t nchunks,
                               uint32_t* __restrict__ chunk_lo, const unsigned long long* __restrict__ dn) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nchunks) return;
    if (dn) n = (uint32_t)min((unsigned long long)n, *dn);  // chunks past the records are empty
    const uint32_t x = c == nchunks ? n : min(c * T, n);
    if (x == 0 || x == n) {
        chunk_lo[2 * c] = x;
        if (c > 0) chunk_lo[2 * c - 1] = x;
        return;
    }
    const uint32_t b = bin_of(q0_mass(recs[x - 1].q0), bm);
    // first i >= x with bin(i) > b (bins are non-decreasing); lo: known <= b
    uint32_t lo = x - 1, step = 1, hi = x;
    while (hi < n && bin_of(q0_mass(recs[hi].q0), bm) <= b) {
        lo = hi;
        step <<= 1;
        hi = min(x - 1 + step, n);
    }
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (bin_of(q0_mass(recs[mid].q0), bm) <= b) lo = mid; else hi = mid;
    }
    chunk_lo[2 * c] = hi;
    constexpr uint32_t BIG = (uint32_t)WAVE_SORT_LIMIT;
    const uint32_t cm = (c - 1) * T;  // a split bin starts at or after (c-1)*T
    uint32_t split = hi;
    if (hi > BIG && bin_of(q0_mass(recs[hi - BIG - 1].q0), bm) == b &&
        bin_of(q0_mass(recs[cm].q0), bm) < b) {
        // more than BIG records, starting after cm: its first record in (cm, hi - BIG - 1]
        uint32_t l2 = cm, u2 = hi - BIG - 1;  // bin(l2) < b, bin(u2) == b
        while (u2 - l2 > 1) {
            const uint32_t mid = l2 + ((u2 - l2) >> 1);
            if (bin_of(q0_mass(recs[mid].q0), bm) < b) l2 = mid; else u2 = mid;
        }
        split = u2;
    }
    chunk_lo[2 * c - 1] = split;
}

hipError_t launch_chunk_bounds(const Rec* d_recs, uint32_t n, const BinMap& bm, uint32_t T, uint32_t nchunks,
                               uint32_t* d_chunk_lo, hipStream_t s, const unsigned long long* d_n) {
    DBI_LAUNCH(k_chunk_bounds, dim3((nchunks + 1 + 255) / 256), dim3(256), 0, s, d_recs, n, bm, T, nchunks,
               d_chunk_lo, d_n);
    return hipGetLastError();
}

// ---- LDS chunk sort over 128-bit keys (k0, k1) = (q0, q1) --------------------
__device__ __forceinline__ bool key_lt(unsigned long long a0, unsigned long long a1, unsigned long long b0,
                                       unsigned long long b1) {
    return (a0 < b0) | ((a0 == b0) & (a1 < b1));
}

__device__ __forceinline__ void cmp_swap(unsigned long long* k0, unsigned long long* k1, uint32_t x, uint32_t y) {
    const unsigned long long a0 = k0[x], b0 = k0[y], a1 = k1[x], b1 = k1[y];
    if (key_lt(b0, b1, a0, a1)) {
        k0[x] = b0; k0[y] = a0;
        k1[x] = b1; k1[y] = a1;
    }
}

// One wave sorts k0/k1[lo, lo+L) in place, ascending, with the all-ascending
// ("flip + half-cleaner") bitonic network over the next power of two: every
// comparator puts the smaller value at the lower index, so the virtual +inf
// padding never moves and comparators that reach past L are simply skipped.
__device__ void wave_bitonic(unsigned long long* k0, unsigned long long* k1, uint32_t lo, uint32_t L) {
    uint32_t P2 = 2;
    while (P2 < L) P2 <<= 1;
    const uint32_t lane = lane_id();
    for (uint32_t k = 2; k <= P2; k <<= 1) {
        const uint32_t half = k >> 1;
        for (uint32_t t = lane; t < (P2 >> 1); t += 64) {
            const uint32_t base = (t / half) * k, off = t & (half - 1);
            const uint32_t l = base + k - 1 - off;
            if (l < L) cmp_swap(k0, k1, lo + base + off, lo + l);
        }
        wave_sync();
        for (uint32_t j = half >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < (P2 >> 1); t += 64) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                if (i + j < L) cmp_swap(k0, k1, lo + i, lo + i + j);
            }
            wave_sync();
        }
    }
}

// The same network with the whole block (runs too big for one wave).
template <int NT>
__device__ void block_bitonic(unsigned long long* k0, unsigned long long* k1, uint32_t lo, uint32_t L) {
    uint32_t P2 = 2;
    while (P2 < L) P2 <<= 1;
    for (uint32_t k = 2; k <= P2; k <<= 1) {
        const uint32_t half = k >> 1;
        for (uint32_t t = threadIdx.x; t < (P2 >> 1); t += NT) {
            const uint32_t base = (t / half) * k, off = t & (half - 1);
            const uint32_t l = base + k - 1 - off;
            if (l < L) cmp_swap(k0, k1, lo + base + off, lo + l);
        }
        __syncthreads();
        for (uint32_t j = half >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < (P2 >> 1); t += NT) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                if (i + j < L) cmp_swap(k0, k1, lo + i, lo + i + j);
            }
            __syncthreads();
        }
    }
}

// ---- compact-key register bitonic (the big bins) ---------------------------
// Inside one fine bin the masses differ in ~32 low bits (bin width ~0.00066 Da
// <= 2^32.4 ulps below 1024 Da), so with mb = mass bits (q0 >> 8) and mb0 the
// run's minimum, one 64-bit key
//   (mb - mb0) << 29 | tag high byte << 21 | tag low byte << 13 | arrival index
// orders a run by (mass, tag), equal (mass, tag) by arrival.  For the device
// digests arrival IS first appearance (records are emitted in protein/offset/
// length order and the radix passes are stable); the order is checked after
// the permutation, and a run that breaks either assumption (mb - mb0 >= 2^35,
// arrival not ascending in q1) is re-sorted by the full 128-bit record key.
// The keys live in registers, R per lane, element i = lane*R + r of the wave
// (w*64R + lane*R + r of the block): the all-ascending flip network, register
// pairs for distances < R, DPP / row swaps above (dbi_lane.h), LDS only across
// waves.
constexpr int CK_IDX_BITS = 13;
constexpr int CK_D_BITS = 64 - 16 - CK_IDX_BITS;

__device__ __forceinline__ bool ck_make(uint64_t q0, uint64_t q1, uint64_t mb0, uint32_t idx, uint64_t& key) {
    const uint64_t d = (q0 >> 8) - mb0;
    key = (d << (16 + CK_IDX_BITS)) | ((q0 & 0xFFu) << (8 + CK_IDX_BITS)) | ((q1 >> 56) << CK_IDX_BITS) | idx;
    return d < (1ull << CK_D_BITS);
}

__device__ __forceinline__ uint64_t ck_q0(uint64_t key, uint64_t mb0) {
    return ((mb0 + (key >> (16 + CK_IDX_BITS))) << 8) | ((key >> (8 + CK_IDX_BITS)) & 0xFFu);
}

__device__ __forceinline__ uint32_t ck_idx(uint64_t key) { return (uint32_t)key & ((1u << CK_IDX_BITS) - 1u); }

// (DPP / row-swap exchanges, dbi_lane.h: no ds_bpermute round trips)
template <bool MAX>
__device__ __forceinline__ uint64_t wave_minmax_u64(uint64_t v) {
    uint64_t o;
    o = lane_xor64<1>(v); v = (o > v) == MAX ? o : v;
    o = lane_xor64<2>(v); v = (o > v) == MAX ? o : v;
    o = lane_xor64<4>(v); v = (o > v) == MAX ? o : v;
    o = lane_xor64<8>(v); v = (o > v) == MAX ? o : v;
    o = lane_xor64<16>(v); v = (o > v) == MAX ? o : v;
    o = lane_xor64<32>(v); v = (o > v) == MAX ? o : v;
    return v;
}
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) { return wave_minmax_u64<false>(v); }
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) { return wave_minmax_u64<true>(v); }

// the network over keys of type T (the 64-bit compact key; 32-bit keys
// compile to v_min / v_max_u32)
template <int M>
__device__ __forceinline__ uint64_t lane_xor_k(uint64_t v) { return lane_xor64<M>(v); }
template <int M>
__device__ __forceinline__ uint32_t lane_xor_k(uint32_t v) { return lane_xor<M>(v); }

template <typename T>
__device__ __forceinline__ void ck_cx(T& a, T& b) {  // a: the lower index
    const T lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

template <typename T>
__device__ __forceinline__ T ck_pick(T a, T b, bool lower) {
    return ((a > b) == lower) ? b : a;  // lower: min, else max
}

// flip step of the K-merge: partner i ^ (K-1)
template <int R, int K, typename T>
__device__ __forceinline__ void ck_flip(T (&key)[R]) {
    if constexpr (K <= R) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < (r ^ (K - 1))) ck_cx(key[r], key[r ^ (K - 1)]);
    } else {
        const bool lower = (lane_id() & (uint32_t)(K / (2 * R))) == 0;
#pragma unroll
        for (int r = 0; r < R / 2; ++r) {  // registers r and R-1-r trade with the partner lane
            const int q = r ^ (R - 1);
            const T br = lane_xor_k<K / R - 1>(key[q]), bq = lane_xor_k<K / R - 1>(key[r]);
            key[r] = ck_pick(key[r], br, lower);
            key[q] = ck_pick(key[q], bq, lower);
        }
    }
}

// half-cleaner step: partner i ^ J
template <int R, int J, typename T>
__device__ __forceinline__ void ck_half(T (&key)[R]) {
    if constexpr (J < R) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < (r ^ J)) ck_cx(key[r], key[r ^ J]);
    } else {
        const bool lower = (lane_id() & (uint32_t)(J / R)) == 0;
#pragma unroll
        for (int r = 0; r < R; ++r) key[r] = ck_pick(key[r], lane_xor_k<J / R>(key[r]), lower);
    }
}

template <int R, int J, typename T>
__device__ __forceinline__ void ck_clean(T (&key)[R]) {
    if constexpr (J >= 1) {
        ck_half<R, J>(key);
        ck_clean<R, J / 2>(key);
    }
}

// sorts the wave's 64R keys ascending (K = 64R at the top)
template <int R, int K, typename T>
__device__ __forceinline__ void ck_sort_wave(T (&key)[R]) {
    if constexpr (K > 2) ck_sort_wave<R, K / 2>(key);
    ck_flip<R, K>(key);
    ck_clean<R, K / 4>(key);
}

// equal (mass, tag) neighbours in [lo+1, lo+L) must ascend in q1 (first appearance)
__device__ __forceinline__ bool ck_order_bad(const unsigned long long* k0, const unsigned long long* k1, uint32_t p) {
    return k0[p] == k0[p - 1] && (k1[p] >> 56) == (k1[p - 1] >> 56) && k1[p] < k1[p - 1];
}

// Records need not arrive in first-appearance order (digest tiles take their
// output regions in arrival order), so after the compact-key sort a run of
// equal (mass, tag) -- the occurrences of one peptide, or a tag collision --
// may be out of q1 order: each run is put in order by one thread (insertion
// sort of q1; q0 is equal across the run).  Runs of [lo, lo+L) whose head
// lies in this thread's share [i0, i1); false when a run is longer than
// CK_RUN_MAX (the caller sorts the whole bin by the full key instead).
constexpr uint32_t CK_RUN_MAX = 32;
__device__ __forceinline__ bool ck_fix_runs(const unsigned long long* k0, unsigned long long* k1, uint32_t lo,
                                            uint32_t L, uint32_t i, uint32_t step) {
    bool ok = true;
    for (; i < L; i += step) {
        if (i > 0 && k0[lo + i] == k0[lo + i - 1] && (k1[lo + i] >> 56) == (k1[lo + i - 1] >> 56)) continue;
        uint32_t e = i + 1;
        while (e < L && k0[lo + e] == k0[lo + i] && (k1[lo + e] >> 56) == (k1[lo + i] >> 56)) ++e;
        if (e - i > CK_RUN_MAX) {
            ok = false;
            continue;
        }
        for (uint32_t a = i + 1; a < e; ++a) {
            const unsigned long long v = k1[lo + a];
            uint32_t b = a;
            for (; b > i && k1[lo + b - 1] > v; --b) k1[lo + b] = k1[lo + b - 1];
            k1[lo + b] = v;
        }
    }
    return ok;
}

// One wave sorts k0/k1[lo, lo+L), L <= 64R, by the compact key; false: the
// run is left a permutation of itself and needs the full-key sort.
// (a call, not inlined: inlined into k_chunk_sort's 64 VGPRs it spills 132 B
// per lane against the call's 28 B of callee-saved registers)
template <int R>
__device__ bool ck_run_wave(unsigned long long* k0, unsigned long long* k1, uint32_t lo, uint32_t L) {
    const uint32_t lane = lane_id();
    uint64_t mb0 = ~0ull;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = lane * R + r;
        if (i < L) {
            const uint64_t o = k0[lo + i] >> 8;
            mb0 = o < mb0 ? o : mb0;
        }
    }
    mb0 = wave_min_u64(mb0);
    uint64_t key[R];
    bool ok = true;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = lane * R + r;
        key[r] = ~0ull;
        if (i < L) ok &= ck_make(k0[lo + i], k1[lo + i], mb0, i, key[r]);
    }
    if (__ballot(!ok)) return false;
    ck_sort_wave<R, 64 * R>(key);
    // q0 comes back out of the key itself; q1 is gathered by the arrival index
    uint64_t g1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = lane * R + r;
        if (i < L) g1[r] = k1[lo + ck_idx(key[r])];
    }
    wave_sync();  // every lane's gather before any write
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = lane * R + r;
        if (i < L) {
            k0[lo + i] = ck_q0(key[r], mb0);
            k1[lo + i] = g1[r];
        }
    }
    wave_sync();
    bool bad = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = lane * R + r;
        if (i > 0 && i < L) bad |= ck_order_bad(k0, k1, lo + i);
    }
    if (__ballot(bad) == 0) return true;
    const bool fixed = ck_fix_runs(k0, k1, lo, L, lane, 64);
    wave_sync();
    return __ballot(!fixed) == 0;
}

// compare-exchange with partner i ^ m across waves, through LDS scratch sc[0, L)
// Element x sits at sig(x): its R-aligned group keeps its place and the low
// bits are xored with bits 5.. of x, so a wave's R stores / loads of one
// register hit 32 distinct 8-B bank pairs (plain lane*R + r strides put R
// lanes on one pair); the group that reaches past L stays unpermuted.
template <int R>
__device__ __forceinline__ uint32_t ck_sig(uint32_t x, uint32_t L) {
    return (x | (uint32_t)(R - 1)) < L ? x ^ ((x >> 5) & (uint32_t)(R - 1)) : x;
}

template <int R>
__device__ __forceinline__ void ck_lds_step(unsigned long long* sc, uint64_t (&key)[R], uint32_t i0, uint32_t m,
                                            uint32_t L) {
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (i0 + r < L) sc[ck_sig<R>(i0 + r, L)] = key[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = i0 + r, p = i ^ m;
        const uint64_t b = p < L ? sc[ck_sig<R>(p, L)] : ~0ull;
        key[r] = ck_pick(key[r], b, i < p);
    }
    __syncthreads();
}

// The whole block sorts k0/k1[lo, lo+L), L <= NT*R, by the compact key (block-
// uniform result; false as in ck_run_wave).  k0[lo, lo+L) is the scratch of the
// cross-wave steps; q0 is rebuilt from the keys.
// s_min: NT/64 slots of scratch.
template <int NT, int R>
__device__ bool ck_run_block(unsigned long long* k0, unsigned long long* k1, uint32_t lo, uint32_t L,
                             uint64_t* s_min) {
    static_assert(NT * R <= (1 << CK_IDX_BITS), "arrival index bits");
    constexpr uint32_t WE = 64 * R;
    const uint32_t i0 = (threadIdx.x >> 6) * WE + lane_id() * R;
    uint64_t mb0 = ~0ull;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (i0 + r < L) {
            const uint64_t o = k0[lo + i0 + r] >> 8;
            mb0 = o < mb0 ? o : mb0;
        }
    mb0 = wave_min_u64(mb0);
    if (lane_id() == 0) s_min[threadIdx.x >> 6] = mb0;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const uint64_t o = s_min[w];
        mb0 = o < mb0 ? o : mb0;
    }
    uint64_t key[R];
    bool ok = true;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        key[r] = ~0ull;
        if (i0 + r < L) ok &= ck_make(k0[lo + i0 + r], k1[lo + i0 + r], mb0, i0 + r, key[r]);
    }
    if (__syncthreads_or(!ok)) return false;
    const bool live = (threadIdx.x >> 6) * WE < L;  // wave-uniform: waves past the run hold +inf only
    if (live) ck_sort_wave<R, WE>(key);
    uint32_t P2 = WE;
    while (P2 < L) P2 <<= 1;
    for (uint32_t k = 2 * WE; k <= P2; k <<= 1) {
        ck_lds_step<R>(k0 + lo, key, i0, k - 1, L);
        for (uint32_t j = k >> 2; j >= WE; j >>= 1) ck_lds_step<R>(k0 + lo, key, i0, j, L);
        if (live) ck_clean<R, WE / 2>(key);
    }
    // q0 comes back out of the key (k0 was the scratch); q1 gathered by arrival index
    uint64_t g1[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (i0 + r < L) g1[r] = k1[lo + ck_idx(key[r])];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (i0 + r < L) {
            k0[lo + i0 + r] = ck_q0(key[r], mb0);
            k1[lo + i0 + r] = g1[r];
        }
    }
    __syncthreads();
    bool bad = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = i0 + r;
        if (i > 0 && i < L) bad |= ck_order_bad(k0, k1, lo + i);
    }
    if (!__syncthreads_or(bad)) return true;
    const bool fixed = ck_fix_runs(k0, k1, lo, L, threadIdx.x, NT);
    return !__syncthreads_or(!fixed);
}

// exclusive max of v over the block's lower threads (0 for thread 0)
template <int NT>
__device__ __forceinline__ uint32_t block_excl_max(uint32_t v, uint32_t* s_tmp) {
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    uint32_t inc = v;  // inclusive max-scan by DPP (0 is the identity), as wave_incl_scan
    inc = max(inc, dpp_or_zero<0x111, 0xF>(inc));
    inc = max(inc, dpp_or_zero<0x112, 0xF>(inc));
    inc = max(inc, dpp_or_zero<0x114, 0xF>(inc));
    inc = max(inc, dpp_or_zero<0x118, 0xF>(inc));
    inc = max(inc, dpp_or_zero<0x142, 0xA>(inc));
    inc = max(inc, dpp_or_zero<0x143, 0xC>(inc));
    if (lane == 63) s_tmp[w] = inc;
    __syncthreads();
    uint32_t r = dpp_or_zero<0x138, 0xF>(inc);  // wave_shr:1 (lane 0: 0)
    for (uint32_t q = 0; q < w; ++q) r = max(r, s_tmp[q]);
    __syncthreads();
    return r;
}

// exclusive min of v over the block's higher threads (`none` for the last)
template <int NT>
__device__ __forceinline__ uint32_t block_excl_min_rev(uint32_t v, uint32_t none, uint32_t* s_tmp) {
    constexpr uint32_t NW = NT / 64;
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_down(inc, d, 64);
        if (lane + d < 64) inc = min(inc, o);
    }
    if (lane == 0) s_tmp[w] = inc;
    __syncthreads();
    uint32_t r = __shfl_down(inc, 1, 64);
    if (lane == 63) r = none;
    for (uint32_t q = w + 1; q < NW; ++q) r = min(r, s_tmp[q]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ bool same_tag_at(const unsigned long long* k0, const unsigned long long* k1, uint32_t p) {
    return k0[p] == k0[p - 1] && (k1[p] >> 56) == (k1[p - 1] >> 56);
}

// Chunk in sorted order in LDS (k0, k1 = the record key): flag unique heads,
// string-verify equal (mass, tag) neighbours, regroup a 16-bit tag collision
// by string (first appearance first), write the records in final order with
// the head flag in the low byte of q0.  aux: scratch (a16[2p] = head info of
// p, a16[2q+1] = q-th verification pair).  Returns this thread's head count.
// p inside one of the nw ranges wr[i] = lo | hi << 16 (bins another kernel sorts)
__device__ __forceinline__ bool in_ranges(const uint32_t* wr, uint32_t nw, uint32_t p) {
    bool in = false;
    for (uint32_t i = 0; i < nw; ++i) in |= p >= (wr[i] & 0xFFFFu) && p < (wr[i] >> 16);
    return in;
}

// wr / nw: record ranges left out (neither written nor counted: the wide bins
// chunk_sort_mid sorts); the record after such a range is in another bin, so
// it is a head whatever the range holds.
template <int NT>
__device__ uint32_t finish_sorted(Rec* __restrict__ out, uint32_t m, const RecLoc& rl, const unsigned long long* k0,
                                  const unsigned long long* k1, uint32_t* aux, uint32_t* s_u32, uint32_t* s_bad,
                                  const uint32_t* wr = nullptr, uint32_t nw = 0, bool raw_skipped = false) {
    uint16_t* a16 = reinterpret_cast<uint16_t*>(aux);
    if (raw_skipped) {  // local bins: the skipped ranges exist only here -- out as they are (tags whole), chunk_sort_mid sorts them there
        for (uint32_t p = threadIdx.x; p < m; p += NT)
            if (in_ranges(wr, nw, p)) out[p] = Rec{k0[p], k1[p]};
    }
    if (threadIdx.x == 0) {
        *s_bad = 0;
        s_u32[NT / 64] = 0;  // number of equal (mass, tag) neighbour pairs
    }
    __syncthreads();
    uint32_t heads = 0;
    for (uint32_t p0 = 0; p0 < m; p0 += NT) {  // wave-uniform trip count: one LDS atomic per wave
        const uint32_t p = p0 + threadIdx.x;
        const bool skip = nw && in_ranges(wr, nw, p);
        const bool dup = p < m && p > 0 && !skip && same_tag_at(k0, k1, p);
        const uint64_t bal = __ballot(dup);
        uint32_t base = 0;
        if (bal && lane_id() == 0) base = atomicAdd(&s_u32[NT / 64], (uint32_t)__popcll(bal));
        base = (uint32_t)__builtin_amdgcn_readlane((int)base, 0);
        if (dup) a16[2 * (base + (uint32_t)__popcll(bal & lanemask_lt())) + 1] = (uint16_t)p;
        if (p < m) {
            a16[2 * p] = (uint16_t)(dup ? 0u : p);
            heads += !dup && !skip;
        }
    }
    __syncthreads();
    // string-verify every pair in one parallel round (each check is a chain
    // of HBM loads: never serialise them per thread)
    const uint32_t npairs = s_u32[NT / 64];
#ifndef DBI_X_NOVERIFY  // (experiment builds: the verification's HBM reads left out -- results not valid)
    for (uint32_t q = threadIdx.x; q < npairs; q += NT) {
        const uint32_t p = a16[2 * q + 1];
        if (!rl.same(Rec{k0[p], k1[p]}, Rec{k0[p - 1], k1[p - 1]})) {
            *s_bad = 1;
            a16[2 * p] = 0x8000u;  // (a dup's head entry is 0) a string boundary inside p's group
        }
    }
#endif
    __syncthreads();
#ifdef DBI_X_NOREGROUP  // (experiment builds: tag collisions left merged -- results not valid)
    if (true) {
#else
    if (*s_bad == 0) {
#endif
        for (uint32_t p = threadIdx.x; p < m; p += NT)
            if (!nw || !in_ranges(wr, nw, p))
                out[p] = Rec{(k0[p] & ~0xFFull) | (a16[2 * p] == p ? 1ull : 0ull), k1[p]};  // p == 0 always a head
        return heads;
    }
    // 16-bit tag collision (block-uniform; SwissProt: ~10 000 per build, the
    // equal (mass, tag) runs of isobaric permutations): group start gs(p) = max
    // head position <= p (block max-scan over contiguous per-thread ranges).
    // Only a group holding a failed pair (bit 15 of its entry, set above) has
    // several strings; every other group is one string (its neighbours
    // verified equal), so its leader is its start, with no string read.
    // aux[p]: bit 31 = a failed pair ends at p; bit 30 (on a group start) =
    // the group holds several strings -- kept through the leader pass below.
    constexpr uint32_t FAILED = 1u << 31, MIXED = 1u << 30;
    {
        const uint32_t E = (m + NT - 1) / NT;
        const uint32_t lo = min(threadIdx.x * E, m), hi = min(lo + E, m);
        uint32_t run = 0;
        for (uint32_t p = lo; p < hi; ++p) run = max(run, (uint32_t)a16[2 * p] & 0x7FFFu);
        uint32_t cur = block_excl_max<NT>(run, s_u32);
        for (uint32_t p = lo; p < hi; ++p) {
            const uint32_t v = a16[2 * p];
            cur = max(cur, v & 0x7FFFu);
            aux[p] = cur | (v & 0x8000u ? FAILED : 0u);  // group start of p (the pair list is dead)
        }
    }
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < m; p += NT)
        if (aux[p] & FAILED) atomicOr(&aux[aux[p] & 0xFFFFu], MIXED);
    __syncthreads();
    // leader = position of the first occurrence of p's string in its group
    // (sorted order inside a group = first appearance); group start kept in
    // bits 16-29
    for (uint32_t p = threadIdx.x; p < m; p += NT) {
        const uint32_t a = aux[p], gs = a & 0xFFFFu;
        uint32_t lead = gs;
        if (aux[gs] & MIXED) {  // (bit 30 of the start's entry survives its rewrite)
            const Rec me{k0[p], k1[p]};
            lead = p;
            for (uint32_t q = gs; q < p; ++q)
                if (rl.same(Rec{k0[q], k1[q]}, me)) { lead = q; break; }
        }
        aux[p] = (a & MIXED) | (gs << 16) | lead;
    }
    __syncthreads();
    heads = 0;
    for (uint32_t p = threadIdx.x; p < m; p += NT) {
        if (nw && in_ranges(wr, nw, p)) continue;  // a head of its own (one-record group), not written
        const uint32_t gs = (aux[p] >> 16) & 0x3FFFu, lead = aux[p] & 0xFFFFu;
        uint32_t np = p;  // a one-string group keeps its order
        if (aux[gs] & MIXED) {
            np = gs;
            for (uint32_t q = gs; q < m && ((aux[q] >> 16) & 0x3FFFu) == gs; ++q) {
                const uint32_t lq = aux[q] & 0xFFFFu;
                np += (lq < lead) | ((lq == lead) & (q < p));
            }
        }
        out[np] = Rec{(k0[p] & ~0xFFull) | (lead == p ? 1ull : 0ull), k1[p]};
        heads += lead == p;
    }
    return heads;
}

// Per chunk (<= CAP records, whole fine mass bins): sort every bin by the
// record key (q0, q1) — mass, peptide tag, first appearance: the pinned unique
// order, independent of the order the records arrive in — then
// finish_sorted().  Bins of <= RANK_MAX_RUN records: each record's rank inside
// its bin from LDS compares (no barriers), scattered from registers; bigger
// bins (equal-mass spikes at SwissProt scale) are sorted in place by the
// compact key in registers (ck_run_wave / ck_run_block), one wave each up to
// WAVE_SORT_MAX, else by the whole block; the full-key bitonic only where the
// compact key does not hold.  LDS: 8+8+4 B per record.
constexpr uint32_t RANK_MAX_RUN = 64;

#ifndef DBI_TAG_SORT
#define DBI_TAG_SORT 1  // single-mass bins above WAVE_SORT_MAX by the tag counting sort (tag_sort_block)
#endif
#ifndef DBI_MID_WPE
#define DBI_MID_WPE 7
#endif
constexpr uint32_t WAVE_SORT_MAX = WAVE_SORT_LIMIT;

template <int NT, int CAP>
struct ChunkSmem {
    static constexpr uint32_t MAXB = CAP / (RANK_MAX_RUN + 1) + 1;  // runs above RANK_MAX_RUN
    static constexpr uint32_t MAXW = CAP / (WAVE_SORT_MAX + 1) + 1;  // runs above WAVE_SORT_MAX
    unsigned long long k0[CAP];
    unsigned long long k1[CAP];
    uint32_t aux[CAP];
    uint32_t big[MAXB];  // lo | hi << 16
    uint32_t wr[MAXW];   // lo | hi << 16: bins left to chunk_sort_mid
    uint32_t u32[NT / 64 + 1];
    uint64_t mins[NT / 64];
    uint64_t maxs[NT / 64];       // local bins: per-wave mass-bit range
    uint16_t tcnt[NT / 64 * 16];  // tag_sort_block: per-wave digit counts, then their scan
    uint32_t nbig, nwide, bad;
};

// local bins of a depth-bin chunk: a power of two >= CAP * DBI_LOCAL_X / 2,
// two 16-bit counters per word in the k0 / k1 arrays (free until the records
// land).  Finer local bins split more of the composition clusters: SwissProt
// records in local bins of <= 64 / 65-512 / > 512 records, 2^10 bins per
// 1 984-record chunk 54 / 36 / 9.6 %, 2^13 64 / 31 / 4.7 %, the limit (2^18)
// 73 / 23 / 3.6 % (tools/depth_sim.py).
#ifndef DBI_LOCAL_X
#define DBI_LOCAL_X 4
#endif
template <int CAP>
constexpr uint32_t local_bins() {
    uint32_t nl = 1;
    while (nl < (uint32_t)CAP * DBI_LOCAL_X / 2) nl <<= 1;
    while (nl * 2u > (uint32_t)CAP * 16u) nl >>= 1;  // inside k0 and k1
    return nl;
}

// Single-mass bins -- equal-mass spikes, every record of the bin with the same
// fp64 mass (isobaric permutations and repeated peptides; the semi-tryptic
// scale's big bins): their order is (16-bit tag, first appearance), so the
// bin is sorted by its tag with four stable 4-bit counting passes over an
// index permutation (wave-ballot ranks in input order, the block's 16 x NW
// digit counts scanned in LDS; O(L) per pass, against the compact-key
// network's O(L log^2 L) with one barrier pair per cross-wave step), the
// records gathered once into that order, then equal-tag runs put in q1
// order (ck_fix_runs).  false (block-uniform): more than one mass in the bin,
// or a run above CK_RUN_MAX (the bin is then a permutation of itself, for the
// caller's compact-key sort).  pa / pb: 2 x L u16 of scratch.
template <int NT, int CAP>
__device__ bool tag_sort_block(unsigned long long* k0, unsigned long long* k1, uint32_t lo, uint32_t L, uint16_t* pa,
                               uint16_t* pb, uint16_t* cnt, uint32_t* s_tmp) {
    constexpr uint32_t NW = NT / 64;
    constexpr uint32_t IT = (CAP + NT - 1) / NT;  // items per lane (a wave's share of L <= CAP)
    static_assert(NW * 16 <= NT, "one scan entry per thread");
    const uint64_t mb = k0[lo] >> 8;
    bool diff = false;
    for (uint32_t i = threadIdx.x; i < L; i += NT) diff |= (k0[lo + i] >> 8) != mb;
    if (__syncthreads_or(diff)) return false;
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    const uint32_t share = (L + NW - 1) / NW;  // wave w ranks positions [w*share, w*share + share)
    const uint32_t wb = min(w * share, L), we = min(wb + share, L);
    uint16_t* src = pa;
    uint16_t* dst = pb;
#pragma unroll 1
    for (uint32_t pass = 0; pass < 4; ++pass) {
        if (lane < 16) cnt[w * 16 + lane] = 0;
        wave_sync();
        // per item: index (13 b) | digit (4 b) << 13 | rank in the wave's digit (15 b) << 17; ~0: none
        uint32_t it[IT];
#pragma unroll
        for (uint32_t k = 0; k < IT; ++k) {
            const uint32_t t = wb + k * 64 + lane;
            const bool valid = t < we;
            const uint32_t j = !valid ? 0u : pass == 0 ? t : (uint32_t)src[t];
            const uint32_t tag = (uint32_t)((k0[lo + j] & 0xFFu) << 8) | (uint32_t)(k1[lo + j] >> 56);
            const uint32_t d = (tag >> (4 * pass)) & 15u;
            const uint64_t peers = digit_peers(d, valid, 4);
            const uint32_t before = cnt[w * 16 + d];
            wave_sync();
            if (valid && (peers & lanemask_lt()) == 0) cnt[w * 16 + d] = (uint16_t)(before + (uint32_t)__popcll(peers));
            wave_sync();
            it[k] = valid ? j | (d << 13) | ((before + (uint32_t)__popcll(peers & lanemask_lt())) << 17) : ~0u;
        }
        __syncthreads();
        // exclusive scan over (digit, wave), digit-major: the first position of
        // wave w's records of digit d
        const uint32_t e = threadIdx.x;  // e = d * NW + ww
        const uint32_t v = e < NW * 16 ? (uint32_t)cnt[(e % NW) * 16 + e / NW] : 0u;
        uint32_t tot;
        const uint32_t base = block_excl_scan<NT, uint32_t>(v, s_tmp, tot);
        if (e < NW * 16) cnt[(e % NW) * 16 + e / NW] = (uint16_t)base;
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < IT; ++k)
            if (it[k] != ~0u) dst[cnt[w * 16 + ((it[k] >> 13) & 15u)] + (it[k] >> 17)] = (uint16_t)(it[k] & 0x1FFFu);
        __syncthreads();
        uint16_t* x = src;
        src = dst;
        dst = x;
    }
    // the records into that order (every read before any write), then runs of equal tags by q1
    // (one word at a time: half the registers; q0 differs only in its tag byte)
    unsigned long long* const kw[2] = {k0, k1};
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        unsigned long long* kk = kw[h];
        unsigned long long v[IT];
#pragma unroll
        for (uint32_t k = 0; k < IT; ++k) {
            const uint32_t t = threadIdx.x + k * NT;
            if (t < L) v[k] = kk[lo + src[t]];
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < IT; ++k) {
            const uint32_t t = threadIdx.x + k * NT;
            if (t < L) kk[lo + t] = v[k];
        }
        __syncthreads();
    }
    const bool fixed = ck_fix_runs(k0, k1, lo, L, threadIdx.x, NT);
    return !__syncthreads_or(!fixed);
}

// The chunk in[0, m) -> out[0, m) in final order with head flags; *heads =
// this thread's unique heads.  BLOCK off: the bins above WAVE_SORT_MAX are
// left out (not written, not counted) and listed in sm.wr[0, sm.nwide) for
// chunk_sort_mid, which sorts each of them on its own (round 3 listed the
// whole chunk, and the mid kernel loaded and ranked it all again).
// ties: records may repeat exactly (host occurrences); ranks count equal keys
// before the record too, so two copies never take one slot.
// LOCAL (depth-bin chunks, whole coarse bins in any order): the bins are the
// chunk's own -- local_bins<CAP>() linear bins over the chunk's mass range
// (block min / max of the mass bits), filled by an LDS counting sort whose
// counters' scan gives every record its place and its bin's bounds at once
// (in place of the fine bins' run detection); the wide bins are written to
// `out` unsorted for chunk_sort_mid.
#ifdef DBI_PHASE_CLOCK  // experiment builds: summed phase cycles of the main chunk sort (dbi_debug_phase_clock)
__device__ unsigned long long g_phase[48];  // [0, 16): main chunk sort, [16, 32): the big tier, [32, 40): its block sorts
#define PHASE_MARK(k) \
    do { if (threadIdx.x == 0) tph[k] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define PHASE_MARK(k) do { } while (0)
#endif
template <int NT, int CAP, bool BLOCK, bool LOCAL = false>
__device__ void sort_chunk(const Rec* __restrict__ in, Rec* __restrict__ out, uint32_t m, const BinMap& bm,
                           const RecLoc& rl, ChunkSmem<NT, CAP>& sm, uint32_t* heads_out, bool ties) {
#ifdef DBI_PHASE_CLOCK
    unsigned long long tph[8] = {};  // (mark 4: after the block-level sorts, BLOCK only)
#endif
    PHASE_MARK(0);
    static_assert(CAP < 16384, "positions in 14 bits (finish_sorted's collision regroup)");
    constexpr uint32_t NW = NT / 64;
    constexpr uint32_t E = (CAP + NT - 1) / NT;  // records per thread (contiguous) in the run pass
    static_assert(E <= 32, "run-head bit mask");
    unsigned long long* k0 = sm.k0;
    unsigned long long* k1 = sm.k1;
    if (threadIdx.x == 0) {
        sm.nbig = 0;
        sm.nwide = 0;
    }
    if constexpr (LOCAL) {
        constexpr uint32_t NL = local_bins<CAP>(), NLW = NL / 2, WPT = (NLW + NT - 1) / NT;
        static_assert(NLW * 4 <= CAP * 16, "the counters inside k0 and k1");
        static_assert(__builtin_offsetof(ChunkSmem<NT, CAP>, k1) == CAP * 8, "k1 right after k0");
        uint32_t* lc = reinterpret_cast<uint32_t*>(k0);  // k0 and k1 are free until the records land
        const uint4* __restrict__ in4 = reinterpret_cast<const uint4*>(in);
        const uint32_t w = threadIdx.x >> 6;
        uint4 rv[E];
#pragma unroll
        for (uint32_t k = 0; k < E; ++k) rv[k] = in4[min(threadIdx.x + k * NT, m - 1u)];  // m >= 1
        for (uint32_t i = threadIdx.x; i < NLW; i += NT) lc[i] = 0;
        uint64_t mn = ~0ull, mx = 0;
#pragma unroll
        for (uint32_t k = 0; k < E; ++k) {
            const uint64_t x = u4_q0(rv[k]) >> 8;  // the clamped duplicates change nothing
            mn = x < mn ? x : mn;
            mx = x > mx ? x : mx;
        }
        mn = wave_min_u64(mn);
        mx = wave_max_u64(mx);
        if (lane_id() == 0) {
            sm.mins[w] = mn;
            sm.maxs[w] = mx;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t q = 0; q < NW; ++q) {
            mn = sm.mins[q] < mn ? sm.mins[q] : mn;
            mx = sm.maxs[q] > mx ? sm.maxs[q] : mx;
        }
        // bin = floor((x - mn) * NL / (range + 1)): non-decreasing in the mass
        const double scale = (double)NL / ((double)(mx - mn) + 1.0);
        uint32_t lr[E];  // local bin << 16 | rank in it (any order)
#pragma unroll
        for (uint32_t k = 0; k < E; ++k) {
            lr[k] = 0;
            if (threadIdx.x + k * NT < m) {
                const uint32_t b = min((uint32_t)((double)((u4_q0(rv[k]) >> 8) - mn) * scale), NL - 1u);
                const uint32_t sh = 16u * (b & 1u);
                lr[k] = (b << 16) | ((atomicAdd(&lc[b >> 1], 1u << sh) >> sh) & 0xFFFFu);
            }
        }
        __syncthreads();
        // exclusive scan of the counters in bin order (each thread WPT
        // consecutive words, read twice rather than held); each word becomes
        // the starts of its two bins
        uint32_t part = 0;
#pragma unroll
        for (uint32_t j = 0; j < WPT; ++j) {
            const uint32_t i = threadIdx.x * WPT + j;
            const uint32_t wd = i < NLW ? lc[i] : 0u;
            part += (wd & 0xFFFFu) + (wd >> 16);
        }
        uint32_t tot;
        uint32_t run = block_excl_scan<NT, uint32_t>(part, sm.u32, tot);
#pragma unroll
        for (uint32_t j = 0; j < WPT; ++j) {
            const uint32_t i = threadIdx.x * WPT + j;
            if (i < NLW) {
                const uint32_t wd = lc[i], lo = wd & 0xFFFFu;
                lc[i] = run | ((run + lo) << 16);
                run += lo + (wd >> 16);
            }
        }
        __syncthreads();
        uint32_t se[E];  // the bin's start | end << 16
#pragma unroll
        for (uint32_t k = 0; k < E; ++k) {
            const uint32_t b = lr[k] >> 16, b1 = b + 1;
            const uint32_t st = (lc[b >> 1] >> (16u * (b & 1u))) & 0xFFFFu;
            const uint32_t en = b1 < NL ? (lc[b1 >> 1] >> (16u * (b1 & 1u))) & 0xFFFFu : m;
            se[k] = st | (en << 16);
        }
        __syncthreads();  // every counter read: k0 takes the records
#pragma unroll
        for (uint32_t k = 0; k < E; ++k) {
            if (threadIdx.x + k * NT < m) {
                const uint32_t st = se[k] & 0xFFFFu, len = (se[k] >> 16) - st, rk = lr[k] & 0xFFFFu;
                k0[st + rk] = u4_q0(rv[k]);
                k1[st + rk] = u4_q1(rv[k]);
                sm.aux[st + rk] = se[k];
                if (rk == 0 && len > RANK_MAX_RUN) {  // one record per bin lists it
                    if (!BLOCK && len > WAVE_SORT_MAX) sm.wr[atomicAdd(&sm.nwide, 1u)] = se[k];
                    else sm.big[atomicAdd(&sm.nbig, 1u)] = se[k];
                }
            }
        }
    } else {
    {
        // all loads in flight before the first use (a Rec as 4 dwords: q0, q1)
        const uint4* __restrict__ in4 = reinterpret_cast<const uint4*>(in);
        uint4 rv[E];
#pragma unroll
        for (uint32_t k = 0; k < E; ++k) {
            const uint32_t i = threadIdx.x + k * NT;
            rv[k] = i < m ? in4[i] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (uint32_t k = 0; k < E; ++k) {
            const uint32_t i = threadIdx.x + k * NT;
            if (i < m) {
                k0[i] = u4_q0(rv[k]);
                k1[i] = u4_q1(rv[k]);
            }
        }
    }
    __syncthreads();
    // bin runs: thread t owns records [t*E, t*E+E); run bounds of each record
    // from a block max-scan (last run start <= i) and a reverse min-scan
    // (first run start > i), kept in registers
    const uint32_t lo0 = threadIdx.x * E;
    uint32_t heads = 0;  // bit k: record lo0+k starts a run
    {
        uint32_t prev = (lo0 > 0 && lo0 - 1 < m) ? bin_of(q0_mass(k0[lo0 - 1]), bm) : ~0u;
#pragma unroll
        for (uint32_t k = 0; k < E; ++k) {
            const uint32_t i = lo0 + k;
            if (i < m) {
                const uint32_t b = bin_of(q0_mass(k0[i]), bm);
                if (i == 0 || b != prev) heads |= 1u << k;
                prev = b;
            }
        }
    }
    {
        uint32_t rlo[E], rhi[E];
        uint32_t cur = block_excl_max<NT>(heads ? lo0 + 31 - __clz(heads) : 0u, sm.u32);
#pragma unroll
        for (uint32_t k = 0; k < E; ++k) {
            if (heads & (1u << k)) cur = lo0 + k;
            rlo[k] = cur;
        }
        cur = block_excl_min_rev<NT>(heads ? lo0 + __ffs(heads) - 1 : m, m, sm.u32);
#pragma unroll
        for (int k = (int)E - 1; k >= 0; --k) {
            rhi[k] = cur;
            if (heads & (1u << k)) cur = lo0 + (uint32_t)k;
        }
#pragma unroll
        for (uint32_t k = 0; k < E; ++k) {
            if ((heads & (1u << k)) && rhi[k] - rlo[k] > RANK_MAX_RUN) {
                if (!BLOCK && rhi[k] - rlo[k] > WAVE_SORT_MAX) sm.wr[atomicAdd(&sm.nwide, 1u)] = rlo[k] | (rhi[k] << 16);
                else sm.big[atomicAdd(&sm.nbig, 1u)] = rlo[k] | (rhi[k] << 16);
            }
            if (lo0 + k < m) sm.aux[lo0 + k] = rlo[k] | (rhi[k] << 16);
        }
    }
    }  // !LOCAL
    __syncthreads();
    PHASE_MARK(1);
    // small bins: rank inside the bin (k-major: a wave's lanes share bins), kept in registers with the key
    // (ranking by a 64-bit compact key instead measured slower: the extra
    // barriers and the order check cost more than the cheaper compares save)
    {
        unsigned long long v0[E], v1[E];
        uint32_t dst[E];
#pragma unroll
        for (uint32_t k = 0; k < E; ++k) {
            const uint32_t i = threadIdx.x + k * NT;
            dst[k] = ~0u;
            const uint32_t bb = i < m ? sm.aux[i] : 0u;
            const uint32_t blo = bb & 0xFFFFu, bhi = bb >> 16;
            if (i < m && bhi - blo <= RANK_MAX_RUN) {
                const unsigned long long a0 = k0[i], a1 = k1[i];
                uint32_t rank = 0;
                if (!ties) {
                    for (uint32_t j = blo; j < bhi; ++j) rank += key_lt(k0[j], k1[j], a0, a1);
                } else {
                    for (uint32_t j = blo; j < bhi; ++j)
                        rank += key_lt(k0[j], k1[j], a0, a1) | ((j < i) & (k0[j] == a0) & (k1[j] == a1));
                }
                v0[k] = a0;
                v1[k] = a1;
                dst[k] = blo + rank;
            }
        }
        __syncthreads();  // every rank read done: scatter the small bins
#pragma unroll
        for (uint32_t k = 0; k < E; ++k) {
            if (dst[k] != ~0u) {
                k0[dst[k]] = v0[k];
                k1[dst[k]] = v1[k];
            }
        }
    }
    PHASE_MARK(2);
    // big bins, in place (disjoint from the small bins)
    const uint32_t nbig = sm.nbig;
    for (uint32_t r = threadIdx.x >> 6; r < nbig; r += NW) {
        const uint32_t b = sm.big[r];
        const uint32_t lo = b & 0xFFFFu, L = (b >> 16) - lo;
        if (L > WAVE_SORT_MAX) continue;
#ifdef DBI_PHASE_CLOCK  // wave-sorted bins: g_phase[44 + BLOCK] count, [46 + BLOCK] single-mass ones
        {
            bool one = true;
            const uint64_t mb = k0[lo] >> 8;
            for (uint32_t i = lane_id(); i < L; i += 64) one &= (k0[lo + i] >> 8) == mb;
            one = __ballot(!one) == 0;
            if (lane_id() == 0) {
                atomicAdd(&g_phase[44 + (BLOCK ? 1 : 0)], 1ull);
                if (one) atomicAdd(&g_phase[46 + (BLOCK ? 1 : 0)], 1ull);
            }
        }
#endif
        bool done;
        if constexpr (WAVE_SORT_MAX > 256)
            done = L <= 128 ? ck_run_wave<2>(k0, k1, lo, L)
                   : L <= 256 ? ck_run_wave<4>(k0, k1, lo, L) : ck_run_wave<8>(k0, k1, lo, L);
        else
            done = L <= 128 ? ck_run_wave<2>(k0, k1, lo, L) : ck_run_wave<4>(k0, k1, lo, L);
        if (!done) wave_bitonic(k0, k1, lo, L);
    }
    __syncthreads();
    PHASE_MARK(3);
    if constexpr (BLOCK) {
        constexpr int R = NT * 4 >= CAP ? 4 : 8;
        static_assert(NT * R >= CAP, "compact-sort capacity");
        uint16_t* a16 = reinterpret_cast<uint16_t*>(sm.aux);  // free until finish_sorted
        for (uint32_t r = 0; r < nbig; ++r) {
            const uint32_t b = sm.big[r];
            const uint32_t lo = b & 0xFFFFu, L = (b >> 16) - lo;
            if (L <= WAVE_SORT_MAX) continue;
            // (the big tier only: in the mid kernel its registers cost a block per CU)
#ifdef DBI_PHASE_CLOCK  // which block-level sort each wide bin took, and its cycles: g_phase[33..39]
            const unsigned long long tb0 = __builtin_amdgcn_s_memtime();
            int path = 0;
            if constexpr (DBI_TAG_SORT && CAP > 2048)
                if (tag_sort_block<NT, CAP>(k0, k1, lo, L, a16, a16 + CAP, sm.tcnt, sm.u32)) path = 1;
            if (!path) path = ck_run_block<NT, R>(k0, k1, lo, L, sm.mins) ? 2 : 3;
            if (path == 3) block_bitonic<NT>(k0, k1, lo, L);
            if (threadIdx.x == 0) {
                atomicAdd(&g_phase[32 + path], 1ull);
                atomicAdd(&g_phase[36 + path], __builtin_amdgcn_s_memtime() - tb0);
                sm.bad = 0;
            }
            __syncthreads();
            // distinct masses of the (now sorted) bin: g_phase[40] sum, [41] bins with <= 16, [42] <= 256, [43] max
            uint32_t dk = 0;
            for (uint32_t i = threadIdx.x; i < L; i += NT) dk += i == 0 || (k0[lo + i] >> 8) != (k0[lo + i - 1] >> 8);
            atomicAdd(&sm.bad, dk);
            __syncthreads();
            if (threadIdx.x == 0) {
                const unsigned long long K = sm.bad;
                atomicAdd(&g_phase[40], K);
                if (K <= 16) atomicAdd(&g_phase[41], 1ull);
                if (K <= 256) atomicAdd(&g_phase[42], 1ull);
                atomicMax(&g_phase[43], K);
            }
            __syncthreads();
            continue;
#endif
            if constexpr (DBI_TAG_SORT && CAP > 2048)
                if (tag_sort_block<NT, CAP>(k0, k1, lo, L, a16, a16 + CAP, sm.tcnt, sm.u32)) continue;
            if (!ck_run_block<NT, R>(k0, k1, lo, L, sm.mins)) block_bitonic<NT>(k0, k1, lo, L);
        }
        __syncthreads();
    }
    PHASE_MARK(4);
    *heads_out = finish_sorted<NT>(out, m, rl, k0, k1, sm.aux, sm.u32, &sm.bad, sm.wr, BLOCK ? 0u : sm.nwide,
                                   LOCAL && !BLOCK);
#ifdef DBI_PHASE_CLOCK
    PHASE_MARK(5);
    if (threadIdx.x == 0) {
        unsigned long long* g = g_phase + (BLOCK ? 16 : 0);
        for (int k = 0; k < 5; ++k) atomicAdd(&g[k], tph[k + 1] - tph[k]);
        atomicAdd(&g[8], 1ull);
        atomicAdd(&g[9], (unsigned long long)m);
        atomicAdd(&g[10], (unsigned long long)sm.nbig);
        atomicAdd(&g[11], (unsigned long long)sm.nwide);
    }
#endif
}

// One chunk of m <= CAP records sorted in LDS by the record key with the flip
// bitonic network (cost independent of how the masses cluster), then
// finish_sorted.  k0/k1/aux: CAP entries each.  Returns this thread's head count.
template <int NT, int CAP>
__device__ uint32_t bitonic_chunk(const Rec* in, Rec* out, uint32_t m, const RecLoc& rl,
                                  unsigned long long* k0, unsigned long long* k1, uint32_t* aux, uint32_t* s_u32,
                                  uint32_t* s_bad, uint64_t* s_min, uint16_t* s_tcnt) {
    static_assert(CAP < 16384, "positions in 14 bits (finish_sorted's collision regroup)");
    for (uint32_t i = threadIdx.x; i < m; i += NT) {
        const Rec r = in[i];
        k0[i] = r.q0;
        k1[i] = r.q1;
    }
    __syncthreads();
    constexpr int R = NT * 4 >= CAP ? 4 : 8;
    static_assert(NT * R >= CAP, "compact-sort capacity");
    // a giant chunk's leaves are mostly one mass (an isobaric spike split by tag bits)
    uint16_t* a16 = reinterpret_cast<uint16_t*>(aux);
    const bool tagged = DBI_TAG_SORT && m > 1 && tag_sort_block<NT, CAP>(k0, k1, 0, m, a16, a16 + CAP, s_tcnt, s_u32);
    if (!tagged && !ck_run_block<NT, R>(k0, k1, 0, m, s_min)) block_bitonic<NT>(k0, k1, 0, m);
    return finish_sorted<NT>(out, m, rl, k0, k1, aux, s_u32, s_bad);
}

// One block per chunk.  A chunk above CAP goes to big_list (k_chunk_sort_list);
// every bin above WAVE_SORT_MAX -- a wide bin inside the chunk, or the
// straddling bin that is chunk c+1 -- to mid_list as (chunk, lo | hi << 16),
// sorted by k_bin_sort_mid, which adds its heads to ucount[chunk].  LDS
// 39 KiB at CAP 1984 and no block-level sort here: <= 64 VGPRs, 4 blocks per CU.

// One chunk c of k_chunk_sort: empty (no heads), above CAP (big_list), or
// sorted here with its wide bins listed for chunk_sort_mid.
template <int NT, int CAP, bool LOCAL>
__device__ void chunk_sort_one(uint32_t c, const Rec* __restrict__ in, Rec* __restrict__ out, const BinMap& bm,
                               const uint32_t* __restrict__ chunk_lo, const RecLoc& rl, uint32_t* __restrict__ ucount,
                               uint32_t* __restrict__ big_list, uint32_t* __restrict__ mid_list, uint32_t ties,
                               Counters* __restrict__ ctr, ChunkSmem<NT, CAP>& sm, bool listed = false) {
    const uint32_t a = chunk_lo[c];
    const uint32_t m = chunk_lo[c + 1] - a;
    if (m == 0) {
        if (threadIdx.x == 0) ucount[c] = 0;
        return;
    }
    if (m > (uint32_t)CAP) {  // (listed: k_depth_chunks put it on big_list already)
        if (threadIdx.x == 0 && !listed) big_list[atomicAdd(&ctr->n_big, 1u)] = c;
        return;
    }
    uint32_t h = 0;
    sort_chunk<NT, CAP, false, LOCAL>(in + a, out + a, m, bm, rl, sm, &h, ties != 0);
    const uint32_t tot = block_sum<NT, uint32_t>(h, sm.u32);
    if (threadIdx.x == 0) ucount[c] = tot;  // block_sum's barrier: before k_bin_sort_mid's adds (stream order)
    if (threadIdx.x < sm.nwide) {
        const uint32_t e = atomicAdd(&ctr->n_mid, 1u);
        mid_list[2 * e] = c;
        mid_list[2 * e + 1] = sm.wr[threadIdx.x];
    }
}

#ifdef DBI_CLOCK_CHUNKS  // experiment builds: per-block clocks of k_chunk_sort (dbi_debug_chunk_clock)
__device__ unsigned long long g_chunk_clock[1u << 18][2];
#endif

// One block per chunk pair (k_chunk_bounds / launch_depth_bounds).  Radix
// tail: chunk 2c here, chunk 2c+1 (one big bin) to the list kernels.  LOCAL
// (depth bins): 2c+1 is empty unless the pair was split; the split ones
// (listed by k_depth_chunks) take the grid's first nfront blocks, so the
// launch starts with its heaviest work instead of ending with it -- when the
// list fits nfront (the previous build's count + a margin); otherwise each
// pair's block sorts its 2c+1 after 2c.  Measured against one block per
// chunk: block b sorting chunk b put every non-empty chunk on every other XCD
// (blocks go to the XCDs round-robin; half the chip idle, 1.76 vs 0.82 ms);
// the even chunks in the grid's first half and the odd ones in its second
// left the split chunks as the launch's tail (1.29-1.31 vs 1.21 ms).
template <int NT, int CAP, bool LOCAL = false>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(8, 8)))
k_chunk_sort(const Rec* __restrict__ in, Rec* __restrict__ out, BinMap bm, const uint32_t* __restrict__ chunk_lo,
             const uint8_t* __restrict__ res, const uint32_t* __restrict__ poff, uint32_t* __restrict__ ucount,
             uint32_t* __restrict__ big_list, uint32_t* __restrict__ mid_list, uint32_t ties,
             Counters* __restrict__ ctr, const uint32_t* __restrict__ split_list, uint32_t nfront, uint32_t listed) {
    __shared__ ChunkSmem<NT, CAP> sm;
    const bool front_ok = LOCAL && ctr->n_split <= nfront;  // block-uniform
    if (LOCAL && blockIdx.x < nfront) {  // a split pair's second chunk, or nothing
        if (!front_ok || blockIdx.x >= ctr->n_split) return;
        const RecLoc rl{res, poff, rec_width(ctr->max_plen)};
        chunk_sort_one<NT, CAP, LOCAL>(2 * split_list[blockIdx.x] + 1, in, out, bm, chunk_lo, rl, ucount, big_list,
                                       mid_list, ties, ctr, sm, listed != 0);
        return;
    }
    const uint32_t c = 2 * (blockIdx.x - (LOCAL ? nfront : 0u));
#ifdef DBI_CLOCK_CHUNKS
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
#endif
    if (!LOCAL && threadIdx.x == 0) {  // chunk c+1: empty, or one big bin for the list kernels
        const uint32_t mb = chunk_lo[c + 2] - chunk_lo[c + 1];
        if (mb == 0) ucount[c + 1] = 0;
        else if (mb > (uint32_t)CAP) big_list[atomicAdd(&ctr->n_big, 1u)] = c + 1;
        else {
            ucount[c + 1] = 0;  // k_bin_sort_mid adds the bin's heads
            const uint32_t e = atomicAdd(&ctr->n_mid, 1u);
            mid_list[2 * e] = c + 1;
            mid_list[2 * e + 1] = mb << 16;
        }
    }
    const RecLoc rl{res, poff, rec_width(ctr->max_plen)};
    chunk_sort_one<NT, CAP, LOCAL>(c, in, out, bm, chunk_lo, rl, ucount, big_list, mid_list, ties, ctr, sm,
                                   listed != 0);
    if constexpr (LOCAL) {
        if (!front_ok || chunk_lo[c + 2] == chunk_lo[c + 1]) {  // (empty: its unique count 0)
            __syncthreads();  // the LDS is the next chunk's
            chunk_sort_one<NT, CAP, LOCAL>(c + 1, in, out, bm, chunk_lo, rl, ucount, big_list, mid_list, ties, ctr,
                                           sm, listed != 0);
        }
    }
#ifdef DBI_CLOCK_CHUNKS
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x < (1u << 18)) {
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        g_chunk_clock[blockIdx.x][0] = t_start | ((t1 - t_start) << 40);
        g_chunk_clock[blockIdx.x][1] = (unsigned long long)(chunk_lo[c + 1] - chunk_lo[c]) |
                                       ((unsigned long long)(chunk_lo[c + 2] - chunk_lo[c + 1]) << 32);
    }
#endif
}

// The big_list chunks k_chunk_sort listed: (CHUNK_CAP, BIG_CAP] records, 1024
// threads, 155 KiB LDS, one block per CU; above split_above they go on to the
// giant path.  One block per listed chunk, blocks past the list exit (a
// grid-stride loop around sort_chunk doubled its registers).
// Two size classes over the one list, as the mid tier: SMALL takes the
// chunks of at most CAP records (and <= split_above) -- 512 threads and half
// the LDS, two blocks per CU (SwissProt: 382 of 421 big chunks, semi-tryptic
// most of them) -- the other class (SMALL false, BIG_CAP) every other entry;
// a block whose entry is the other class's skips it.
template <int NT, int CAP, bool SMALL = false, bool LOCAL = false>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4, 8)))
k_chunk_sort_list(const Rec* __restrict__ in, Rec* __restrict__ out, BinMap bm, const uint32_t* __restrict__ chunk_lo,
                  const uint8_t* __restrict__ res, const uint32_t* __restrict__ poff, uint32_t* __restrict__ ucount,
                  const uint32_t* __restrict__ list, uint32_t* __restrict__ giant_list, uint32_t split_above,
                  uint32_t ties, Counters* __restrict__ ctr, uint32_t small_cap) {
    __shared__ ChunkSmem<NT, CAP> sm;
    const uint32_t n = ctr->n_big;
    if (blockIdx.x == 0 && threadIdx.x == 0 && n > gridDim.x) atomicOr(&ctr->err, ERR_GRID);
    const RecLoc rl{res, poff, rec_width(ctr->max_plen)};
    const uint32_t j = blockIdx.x;
    // the small class's entries: at most small_cap (<= its CAP) and split_above records
    auto small_entry = [&](uint32_t m) { return m <= small_cap && m <= split_above; };
    const uint32_t mj = j < n ? chunk_lo[list[j] + 1] - chunk_lo[list[j]] : 0u;
    if (j < n && small_entry(mj) == SMALL) {
        const uint32_t c = list[j];
        const uint32_t a = chunk_lo[c];
        const uint32_t m = chunk_lo[c + 1] - a;
        if (m > split_above && giant_list) {
            if (threadIdx.x == 0) {
                giant_list[atomicAdd(&ctr->n_giant, 1u)] = c;
                atomicAdd(&ctr->n_giant_recs, (unsigned long long)m);
            }
        } else if (m > split_above) {
            // no giant pass this build (none last time): through unsorted, redone (ERR_GRID)
            for (uint32_t i = threadIdx.x; i < m; i += NT) out[a + i] = Rec{in[a + i].q0 & ~0xFFull, in[a + i].q1};
            if (threadIdx.x == 0) {
                ucount[c] = 0;
                atomicOr(&ctr->err, ERR_GRID);
            }
        } else {
            uint32_t h = 0;
            sort_chunk<NT, CAP, true, LOCAL>(in + a, out + a, m, bm, rl, sm, &h, ties != 0);
            const uint32_t tot = block_sum<NT, uint32_t>(h, sm.u32);
            if (threadIdx.x == 0) {
                ucount[c] = tot;
                atomicAdd(&ctr->n_big_recs, (unsigned long long)m);
            }
        }
    }
    // entries past the grid (ERR_GRID: the build is redone with full grids):
    // their records go to `out` unsorted and without unique heads, so the rest
    // of this build stays inside its buffers
    for (uint32_t e = j + gridDim.x; e < n; e += gridDim.x) {
        const uint32_t c = list[e];
        const uint32_t a = chunk_lo[c];
        const uint32_t m = chunk_lo[c + 1] - a;
        if (small_entry(m) != SMALL) continue;
        for (uint32_t i = threadIdx.x; i < m; i += NT) out[a + i] = Rec{in[a + i].q0 & ~0xFFull, in[a + i].q1};
        if (threadIdx.x == 0) ucount[c] = 0;
    }
}

// The mid_list bins: one fine bin of (WAVE_SORT_MAX, CHUNK_CAP] records per
// entry (chunk, lo | hi << 16), one block each: loaded alone, sorted as one
// run (tag counting sort for a single-mass bin, else the block-level compact
// sort), heads added to ucount[chunk].  No run detection, no small-bin pass:
// the chunk's other records were finished by k_chunk_sort.
// Two size classes over the one list (LMIN < L <= CAP each; a block whose
// entry is the other class's skips it): bins of up to 1024 records
// in 256-thread blocks with half the LDS -- 7 blocks per CU instead of 4
// (5 728 of SwissProt's 7 310 mid bins) -- the rest in 512-thread blocks.
template <int NT, int CAP, uint32_t LMIN>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(DBI_MID_WPE, 8)))
k_bin_sort_mid(const Rec* in, Rec* out, const uint32_t* __restrict__ chunk_lo,  // in == out: depth-bin builds
               const uint8_t* __restrict__ res, const uint32_t* __restrict__ poff, uint32_t* __restrict__ ucount,
               const uint32_t* __restrict__ list, Counters* __restrict__ ctr) {
    __shared__ unsigned long long k0[CAP];
    __shared__ unsigned long long k1[CAP];
    __shared__ uint32_t aux[CAP];
    __shared__ uint32_t s_u32[NT / 64 + 1];
    __shared__ uint64_t s_min[NT / 64];
    __shared__ uint16_t s_tcnt[NT / 64 * 16];
    __shared__ uint32_t s_bad;
    const uint32_t n = ctr->n_mid;
    if (blockIdx.x == 0 && threadIdx.x == 0 && n > gridDim.x) atomicOr(&ctr->err, ERR_GRID);
    const uint32_t j = blockIdx.x;
    const uint32_t Lj = j < n ? (list[2 * j + 1] >> 16) - (list[2 * j + 1] & 0xFFFFu) : 0u;
    if (j < n && Lj > LMIN && Lj <= (uint32_t)CAP) {  // else the other class's entry (block-uniform)
        const uint32_t c = list[2 * j], r = list[2 * j + 1];
        const uint32_t a = chunk_lo[c] + (r & 0xFFFFu), L = (r >> 16) - (r & 0xFFFFu);
        const RecLoc rl{res, poff, rec_width(ctr->max_plen)};
        const uint32_t h = bitonic_chunk<NT, CAP>(in + a, out + a, L, rl, k0, k1, aux, s_u32, &s_bad, s_min, s_tcnt);
        const uint32_t tot = block_sum<NT, uint32_t>(h, s_u32);
        if (threadIdx.x == 0) {
            atomicAdd(&ucount[c], tot);
            atomicAdd(&ctr->n_mid_recs, (unsigned long long)L);
        }
    }
    // entries past the grid (ERR_GRID, redone): the bin unsorted, no heads
    for (uint32_t e = j + gridDim.x; e < n && in != out; e += gridDim.x) {
        const uint32_t c = list[2 * e], r = list[2 * e + 1];
        const uint32_t a = chunk_lo[c] + (r & 0xFFFFu), L = (r >> 16) - (r & 0xFFFFu);
        if (L <= LMIN || L > (uint32_t)CAP) continue;
        for (uint32_t i = threadIdx.x; i < L; i += NT) out[a + i] = Rec{in[a + i].q0 & ~0xFFull, in[a + i].q1};
    }
}

hipError_t launch_chunk_sort(const Rec* d_in, Rec* d_out, const BinMap& bm, const uint32_t* d_chunk_lo,
                             uint32_t nchunks, const uint8_t* d_res, const uint32_t* d_poff, uint32_t* d_ucount,
                             uint32_t* d_big_list, uint32_t* d_mid_list, bool ties, Counters* d_ctr, hipStream_t s,
                             bool local, const uint32_t* d_split_list, uint32_t nfront, bool big_listed) {
    if (nchunks == 0) return hipSuccess;
    if (local && nfront && !d_split_list) return hipErrorInvalidValue;
    if (big_listed && !local) return hipErrorInvalidValue;  // (only k_depth_chunks lists the big chunks)
    if (local)
        DBI_LAUNCH((k_chunk_sort<CHUNK_THREADS, CHUNK_CAP, true>), dim3(nfront + nchunks), dim3(CHUNK_THREADS), 0, s,
                   d_in, d_out, bm, d_chunk_lo, d_res, d_poff, d_ucount, d_big_list, d_mid_list, ties ? 1u : 0u, d_ctr,
                   d_split_list, nfront, big_listed ? 1u : 0u);
    else
        DBI_LAUNCH((k_chunk_sort<CHUNK_THREADS, CHUNK_CAP>), dim3(nchunks), dim3(CHUNK_THREADS), 0, s, d_in,
                   d_out, bm, d_chunk_lo, d_res, d_poff, d_ucount, d_big_list, d_mid_list, ties ? 1u : 0u, d_ctr,
                   (const uint32_t*)nullptr, 0u, 0u);
    return hipGetLastError();
}

#ifdef DBI_PHASE_CLOCK
}  // namespace dbi
extern "C" int dbi_debug_phase_clock(unsigned long long* out, int reset) {
    if (reset) {
        unsigned long long z[48] = {};
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(dbi::g_phase), z, sizeof(z), 0, hipMemcpyHostToDevice);
    }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(dbi::g_phase), 48 * 8, 0, hipMemcpyDeviceToHost);
}
namespace dbi {
#endif

#ifdef DBI_DIGEST_CLOCK
}  // namespace dbi
extern "C" int dbi_debug_digest_clock(unsigned long long* out, int reset) {
    if (reset) {
        unsigned long long z[16] = {};
        return (int)hipMemcpyToSymbol(HIP_SYMBOL(dbi::g_dphase), z, sizeof(z), 0, hipMemcpyHostToDevice);
    }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(dbi::g_dphase), 16 * 8, 0, hipMemcpyDeviceToHost);
}
namespace dbi {
#endif

#ifdef DBI_CLOCK_CHUNKS
}  // namespace dbi
extern "C" int dbi_debug_chunk_clock(unsigned long long* out, unsigned long long n) {
    if (n > (1ull << 18)) n = 1ull << 18;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(dbi::g_chunk_clock), n * 16, 0, hipMemcpyDeviceToHost);
}
namespace dbi {
#endif

hipError_t launch_chunk_sort_mid(const Rec* d_in, Rec* d_out, const BinMap& bm, const uint32_t* d_chunk_lo,
                                 const uint8_t* d_res, const uint32_t* d_poff, uint32_t* d_ucount,
                                 const uint32_t* d_mid_list, uint32_t max_blocks, Counters* d_ctr, hipStream_t s) {
    if (max_blocks == 0) return hipSuccess;
    (void)bm;
    constexpr uint32_t MID_SPLIT = 1024;  // bins of (WAVE_SORT_MAX, MID_SPLIT] records: the small-block class
    static_assert(MID_SPLIT > WAVE_SORT_MAX && MID_SPLIT < CHUNK_CAP, "mid size classes");
    DBI_LAUNCH((k_bin_sort_mid<MID_SPLIT / 4, MID_SPLIT, WAVE_SORT_MAX>), dim3(max_blocks), dim3(MID_SPLIT / 4), 0, s,
               d_in, d_out, d_chunk_lo, d_res, d_poff, d_ucount, d_mid_list, d_ctr);
    DBI_LAUNCH((k_bin_sort_mid<CHUNK_THREADS, CHUNK_CAP, MID_SPLIT>), dim3(max_blocks), dim3(CHUNK_THREADS), 0, s, d_in, d_out,
               d_chunk_lo, d_res, d_poff, d_ucount, d_mid_list, d_ctr);
    return hipGetLastError();
}

constexpr uint32_t BIG_SPLIT_CUS = 256;  // MI355X compute units
hipError_t launch_chunk_sort_big(const Rec* d_in, Rec* d_out, const BinMap& bm, const uint32_t* d_chunk_lo,
                                 const uint8_t* d_res, const uint32_t* d_poff, uint32_t* d_ucount,
                                 const uint32_t* d_big_list, uint32_t* d_giant_list, uint32_t max_blocks,
                                 uint32_t split_above, bool ties, Counters* d_ctr, hipStream_t s, int split_mode,
                                 bool local) {
    if (max_blocks == 0) return hipSuccess;
    constexpr int SMALL_BIG = BIG_CAP / 2;  // 3968 records: 512 threads, 2 blocks per CU
    const uint32_t sa = std::min<uint32_t>(split_above, (uint32_t)BIG_CAP);
    // the two classes only for long lists: a few hundred big chunks (SwissProt
    // tryptic: 421) take two rounds of the 1024-thread blocks either way, and the
    // second launch's skipping blocks cost more than the small class saves
    // (0.15 -> 0.24 ms measured); semi-tryptic's ~70 k: 18.0 -> 15.4 ms
    // (split_mode: DBI_BIG_SPLIT, 0 never / 1 always, for the tests; -1 by the list length)
    const bool split = split_mode < 0 ? max_blocks > 4u * BIG_SPLIT_CUS : split_mode != 0;
#define DBI_BIG_LAUNCH(LOC)                                                                                          \
    do {                                                                                                             \
        if (split)                                                                                                   \
            DBI_LAUNCH((k_chunk_sort_list<BIG_THREADS / 2, SMALL_BIG, true, LOC>), dim3(max_blocks),                 \
                       dim3(BIG_THREADS / 2), 0, s, d_in, d_out, bm, d_chunk_lo, d_res, d_poff, d_ucount, d_big_list, \
                       d_giant_list, sa, ties ? 1u : 0u, d_ctr, (uint32_t)SMALL_BIG);                                \
        DBI_LAUNCH((k_chunk_sort_list<BIG_THREADS, BIG_CAP, false, LOC>), dim3(max_blocks), dim3(BIG_THREADS), 0, s, \
                   d_in, d_out, bm, d_chunk_lo, d_res, d_poff, d_ucount, d_big_list, d_giant_list, sa,               \
                   ties ? 1u : 0u, d_ctr, split ? (uint32_t)SMALL_BIG : 0u);                                         \
    } while (0)
    if (local) DBI_BIG_LAUNCH(true);
    else DBI_BIG_LAUNCH(false);
#undef DBI_BIG_LAUNCH
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// inline '[formula]' PTMs (DBIndexer.java:288-303): the proteins that carry
// them, one thread each, walked literally.  The first start whose walk reaches
// a formula adds its mass as one more step (pepSize + 1, the residue before it
// counted again by isEnzyme and checkCleavage, :295-318) and removes it from
// the protein; every later start sees the protein without it.  Here the
// protein is given stripped (sres) with its formulas as events (position in
// the stripped protein = index of the residue that followed ']'; mass, NaN for
// an unknown element: the exception ends the protein, :400-403), and the
// pending events stand in for the '[' characters checkCleavage still sees.
// Peptide identity (tag, later the string verification) is the protein as
// stored in the ProteinCache -- with its formulas -- at the stripped offsets
// (IndexMerge reads getPeptideSequence(protId, offset, length), :452).
// COUNT: kept records per protein; EMIT: the records at base[i], counters.
// ---------------------------------------------------------------------------
template <bool EMIT>
__global__ void __launch_bounds__(64)
k_ptm_digest(DevParams dp, const double* __restrict__ mass_tab, const uint8_t* __restrict__ flags_tab,
             const uint8_t* __restrict__ sres, const uint32_t* __restrict__ soff, const uint8_t* __restrict__ ores,
             const uint32_t* __restrict__ ooff, const uint32_t* __restrict__ ptm_pid,
             const uint32_t* __restrict__ ev_off, const uint32_t* __restrict__ ev_pos,
             const double* __restrict__ ev_mass, uint32_t n_ptm, uint32_t* __restrict__ cnt,
             Rec* __restrict__ out, Counters* __restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ptm) return;
    const uint8_t* __restrict__ T = sres + soff[i];
    const uint32_t Ls = soff[i + 1] - soff[i];
    const uint32_t pid = ptm_pid[i];
    const uint8_t* __restrict__ O = ores + ooff[pid];
    const uint32_t eb = ev_off[i], ee = ev_off[i + 1];
    const uint32_t w = rec_width(ctr->max_plen);
    Rec* __restrict__ o = EMIT ? out + cnt[i] : nullptr;  // EMIT: cnt holds the exclusive offsets
    const bool can_drop = dp.drop_mass <= dp.max_mh;
    uint32_t kept = 0, dropped = 0;
    uint32_t k = eb;  // first formula not yet removed
    bool dead = false;
    for (uint32_t s = 0; s < Ls && !dead; ++s) {
        double m = dp.m0;                  // :265-271
        int mc = -1;                       // :280
        uint32_t pep = 0;                  // pepSize
        uint32_t p = s;                    // next residue
        bool mand_all = false, mand_excl = false;  // mandatory residue in [s, p) / [s, p-1)
        uint32_t focc = 0;                 // peptide filter, kind 1: counted residues in [s, p)
        while (m <= dp.max_mh) {           // :284 (end < length below)
            uint32_t q;                    // end: the peptide's last residue
            if (k < ee && ev_pos[k] == p) {  // '[' at end (:288-303)
                const double f = ev_mass[k];
                if (!(f == f)) {
                    dead = true;
                    break;
                }
                ++pep;
                m = m + f;
                ++k;
                q = p - 1;
            } else {
                if (p >= Ls) break;
                // the peptide filter sees the stripped residues [s, p] (:309-313; a formula step
                // appends nothing to pepSeq and asks about the same string again: no new answer)
                if (dp.pf_kind && filter_breaks(dp, flags_tab[T[p]], soff[i] + s, soff[i] + p, focc)) break;
                ++pep;
                m = m + mass_tab[T[p]];    // :306-308
                q = p;
                ++p;
                mand_excl = mand_all;
                mand_all = mand_all || (flags_tab[T[q]] & F_MAND) != 0;
            }
            const uint8_t fq = flags_tab[T[q]];
            mc += (fq & F_CLEAVE) ? 1 : 0;  // isEnzyme(protSeq.charAt(end)) (:314-316)
            // checkCleavage over the current protein: a pending formula right
            // after end is a '[' (no cleave / no-cut residue), and end is the
            // protein's last character only with no formula after it
            const bool nxt_f = k < ee && ev_pos[k] == q + 1;
            const bool n_ok = s == 0 || ((flags_tab[T[s - 1]] & F_CLEAVE) && !(flags_tab[T[s]] & F_NOCUT));
            const bool c_ok = (q + 1 == Ls && !nxt_f) ||
                              ((fq & F_CLEAVE) && (nxt_f || q + 1 >= Ls || !(flags_tab[T[q + 1]] & F_NOCUT)));
            const bool cut = dp.semi ? (n_ok || c_ok) : (n_ok && c_ok);  // :318
            if (!cut) continue;
            if (mc > dp.max_missed) break;     // :322-324
            if (m > dp.max_mh) break;          // :326-329
            if (!(pep >= (uint32_t)dp.min_len && m >= dp.min_mh)) continue;  // :331
            if (dp.mand_mode && !mand_all) break;  // :334-344
            bool keep = !dp.mand_filter || mand_excl;  // filterSequence (SQLiteMult :245-268)
            if (dp.filter) {                   // MassRangeFilteringIndex.filterSequence
                if (m > dp.win_max) break;     // SKIP_PROTEIN_START (:351-354)
                keep = keep && in_windows(dp, m);
            }
            if (!keep) continue;
            if (can_drop && m >= dp.drop_mass) {  // bucket > NUM_BUCKETS-1 (SQLiteMult :282-288)
                ++dropped;
                continue;
            }
            if (EMIT) {
                const uint32_t len = q - s + 1;  // curSeqI
                const uint32_t tag = peptide_tag_of(O + s, len);
                o[kept] = Rec{rec_q0(m, tag), rec_q1(tag, rec_loc(pid, s, w), len)};
            }
            ++kept;
        }
    }
    if (!EMIT) {
        cnt[i] = kept;
    } else {
        if (kept) atomicAdd(&ctr->n_kept, (unsigned long long)kept);
        if (dropped) atomicAdd(&ctr->n_dropped, (unsigned long long)dropped);
    }
}

hipError_t launch_ptm_digest(bool emit, const DevParams& dp, const double* d_mass_tab, const uint8_t* d_flags,
                             const uint8_t* d_sres, const uint32_t* d_soff, const uint8_t* d_ores,
                             const uint32_t* d_ooff, const uint32_t* d_pid, const uint32_t* d_ev_off,
                             const uint32_t* d_ev_pos, const double* d_ev_mass, uint32_t n_ptm, uint32_t* d_cnt,
                             Rec* d_out, Counters* d_ctr, hipStream_t s) {
    if (n_ptm == 0) return hipSuccess;
    const dim3 g((n_ptm + 63) / 64);
    if (emit)
        DBI_LAUNCH(k_ptm_digest<true>, g, dim3(64), 0, s, dp, d_mass_tab, d_flags, d_sres, d_soff, d_ores, d_ooff,
                   d_pid, d_ev_off, d_ev_pos, d_ev_mass, n_ptm, d_cnt, d_out, d_ctr);
    else
        DBI_LAUNCH(k_ptm_digest<false>, g, dim3(64), 0, s, dp, d_mass_tab, d_flags, d_sres, d_soff, d_ores, d_ooff,
                   d_pid, d_ev_off, d_ev_pos, d_ev_mass, n_ptm, d_cnt, d_out, d_ctr);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// 6. finalize: unique table + occurrence CSR (per chunk)
// ---------------------------------------------------------------------------
// Per chunk: protein id of every occurrence (occurrence CSR, insertion order
// inside each unique peptide) and the unique table at the head records.
// A round covers FIN_ITEMS * FIN_THREADS records, k-major (record
// t0 + k*NT + tid), so every load/store instruction is coalesced and all loads
// of a round are in flight together; unique slots come from per-(k, wave)
// ballot counts.  Protein id, offset and length come out of the record itself.
// 256 threads x 8 records a round: one round covers a whole chunk (1280-1536
// records, pairs up to ~2000); 256 x 4 took two rounds for most chunks
// (SwissProt finalize 0.44 -> 0.40 ms, semi-tryptic 8.6 -> 7.8 ms; 512 x 4
// is as fast at SwissProt scale but not at semi's; DBI_FIN picks another
// shape for A/B)
template <uint32_t FIN_THREADS, uint32_t FIN_ITEMS>
__global__ void __launch_bounds__(FIN_THREADS)
k_finalize(const Rec* __restrict__ recs, const uint32_t* __restrict__ chunk_lo, const uint32_t* __restrict__ ubase,
           double* __restrict__ umass, uint32_t* __restrict__ upid, uint32_t* __restrict__ uoff,
           uint32_t* __restrict__ ulen, uint32_t* __restrict__ occ_off, uint32_t* __restrict__ occ_pid,
           int32_t factor, uint32_t ucap, uint32_t cstride, uint32_t n_kept,
           const unsigned long long* __restrict__ dn, Counters* __restrict__ ctr) {
    constexpr uint32_t NW = FIN_THREADS / 64;
    // the CSR's closing offset (occ_off holds n_kept + 1 entries; a unique
    // count past that is never written)
    if (blockIdx.x == 0 && threadIdx.x == 0 && ctr->n_unique <= n_kept)
        occ_off[ctr->n_unique] = dn ? (uint32_t)*dn : n_kept;
    __shared__ uint32_t wc[FIN_ITEMS * NW];  // heads per (round item k, wave), then exclusive bases
    __shared__ uint32_t s_tot;
    const uint32_t c = blockIdx.x;
    const uint32_t a = chunk_lo[cstride * c];  // a chunk pair (cstride 2) is one contiguous range
    const uint32_t n = chunk_lo[cstride * (c + 1)] - a;
    const uint32_t W = rec_width(ctr->max_plen);
    const uint4* __restrict__ r4 = reinterpret_cast<const uint4*>(recs + a);
    const uint32_t w = threadIdx.x >> 6;
    uint32_t run = ubase[cstride * c];
    uint32_t nkeys = 0;  // heads whose mass key differs from the previous unique's (SQLiteByte rows)
    for (uint32_t t0 = 0; t0 < n; t0 += FIN_THREADS * FIN_ITEMS) {
        uint4 rv[FIN_ITEMS];
        uint32_t lpre[FIN_ITEMS];
        // lane 0 also needs the record before its own (the rest take it from
        // the lane below).  Loads at clamped indices, no branches: every load
        // of the round in flight together (a load per branch costs one round
        // trip each); lanes past the chunk drop what they read.
        const bool l0 = lane_id() == 0;
        unsigned long long pq[FIN_ITEMS];
#pragma unroll
        for (uint32_t k = 0; k < FIN_ITEMS; ++k) {
            const uint32_t i = t0 + k * FIN_THREADS + threadIdx.x;
            const uint32_t ic = min(i, n - 1);
            const uint32_t ip = a + ic > 0 ? a + ic - 1 : 0u;
            rv[k] = r4[ic];  // low byte of q0 = head flag (hd below: only below n)
            pq[k] = recs[l0 ? ip : a + ic].q0;  // lanes > 0: the line they already read
        }
        bool hd[FIN_ITEMS];
#pragma unroll
        for (uint32_t k = 0; k < FIN_ITEMS; ++k) hd[k] = t0 + k * FIN_THREADS + threadIdx.x < n && (rv[k].x & 0xFFu);
        // mass of the record before each head (= the previous unique's mass)
        double prevm[FIN_ITEMS];
#pragma unroll
        for (uint32_t k = 0; k < FIN_ITEMS; ++k) {
            const uint32_t i = t0 + k * FIN_THREADS + threadIdx.x;
            const uint32_t px = __shfl_up((int)rv[k].x, 1, 64), py = __shfl_up((int)rv[k].y, 1, 64);
            const unsigned long long prev = l0 ? pq[k] : (((unsigned long long)py << 32) | px);
            prevm[k] = (hd[k] && a + i > 0) ? q0_mass(prev) : 0.0;
        }
#pragma unroll
        for (uint32_t k = 0; k < FIN_ITEMS; ++k) {
            const uint64_t bal = __ballot(hd[k]);
            lpre[k] = (uint32_t)__popcll(bal & lanemask_lt());
            if (lane_id() == 0) wc[k * NW + w] = (uint32_t)__popcll(bal);
        }
        __syncthreads();
        if (threadIdx.x < 64) {  // exclusive scan of the (k, wave) head counts in wave 0
            constexpr uint32_t NQ = FIN_ITEMS * NW;
            static_assert(NQ <= 64, "one lane per (k, wave)");
            const uint32_t v = threadIdx.x < NQ ? wc[threadIdx.x] : 0u;
            uint32_t incl = v;
#pragma unroll
            for (uint32_t d = 1; d < NQ; d <<= 1) {
                const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
                if (threadIdx.x >= d) incl += o;
            }
            if (threadIdx.x < NQ) wc[threadIdx.x] = incl - v;
            if (threadIdx.x == NQ - 1) s_tot = incl;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < FIN_ITEMS; ++k) {
            const uint32_t i = t0 + k * FIN_THREADS + threadIdx.x;
            if (i < n) {
                const uint64_t q1 = u4_q1(rv[k]);
                const uint32_t pid = q1_pid(q1, W);
                occ_pid[a + i] = pid;
                const uint32_t u = run + wc[k * NW + w] + lpre[k];
                if (hd[k] && u < ucap) {  // (always below ucap; never a write past the table)
                    const double mu = u4_mass(rv[k]);
                    nkeys += (a + i == 0) || java_d2i(mu * (double)factor) != java_d2i(prevm[k] * (double)factor);
                    umass[u] = mu;
                    upid[u] = pid;
                    uoff[u] = q1_off(q1, W);
                    ulen[u] = q1_len(q1, W);
                    occ_off[u] = a + i;
                }
            }
        }
        run += s_tot;
        __syncthreads();  // wc / s_tot reused next round
    }
    const uint32_t t = block_sum<FIN_THREADS, uint32_t>(nkeys, wc);
    // one add per block into one of 8 shards (no single-word contention)
    if (threadIdx.x == 0 && t) atomicAdd(&ctr->n_keys_shard[blockIdx.x & 7], (unsigned long long)t);
}

hipError_t launch_finalize(const Rec* d_recs, const uint32_t* d_chunk_lo, uint32_t nchunks, const uint32_t* d_ubase,
                           double* d_umass, uint32_t* d_upid, uint32_t* d_uoff, uint32_t* d_ulen,
                           uint32_t* d_occ_off, uint32_t* d_occ_pid, int32_t factor, uint32_t ucap, uint32_t cstride,
                           uint32_t n_kept, const unsigned long long* d_n, Counters* d_ctr, hipStream_t s) {
    if (nchunks == 0) return launch_write_tail(d_occ_off, n_kept, d_ctr, s, d_n);
#define DBI_FIN_LAUNCH(NT, K)                                                                                  \
    DBI_LAUNCH((k_finalize<NT, K>), dim3(nchunks), dim3(NT), 0, s, d_recs, d_chunk_lo, d_ubase, d_umass, d_upid, \
               d_uoff, d_ulen, d_occ_off, d_occ_pid, factor, ucap, cstride, n_kept, d_n, d_ctr)
    DBI_FIN_LAUNCH(256, 8);  // (256 x 4, round 3's shape, and 512 x 4 measured slower: DESIGN.md §6 round 4)
#undef DBI_FIN_LAUNCH
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// flags[i] = 1 where the mass key (int)(mass*factor) of unique i differs from
// unique i-1's (dbi_entry_keys; the count itself comes from k_finalize)
__global__ void k_key_flags(const double* __restrict__ umass, uint32_t n, int32_t factor,
                            uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    flags[i] = (i == 0) || (java_d2i(umass[i - 1] * (double)factor) != java_d2i(umass[i] * (double)factor));
}

hipError_t launch_key_flags(const double* d_umass, uint32_t n_unique, int32_t factor, uint32_t* d_flags,
                            hipStream_t s) {
    if (n_unique == 0) return hipSuccess;
    DBI_LAUNCH(k_key_flags, dim3((n_unique + 255) / 256), dim3(256), 0, s, d_umass, n_unique, factor, d_flags);
    return hipGetLastError();
}

// occ_off[U] = n_kept (U from the device counters)
__global__ void k_tail_counts(Counters* __restrict__ ctr, uint64_t cap, int sparse) {
    if (threadIdx.x != 0) return;
    const unsigned long long need = sparse ? ctr->n_slots : ctr->n_kept;
    const bool fit = need <= cap;
    ctr->tail_in = fit ? need : 0ull;
    ctr->tail_n = fit ? ctr->n_kept : 0ull;
}

hipError_t launch_tail_counts(Counters* d_ctr, uint64_t cap, bool sparse, hipStream_t s) {
    DBI_LAUNCH(k_tail_counts, dim3(1), dim3(64), 0, s, d_ctr, cap, sparse ? 1 : 0);
    return hipGetLastError();
}

__global__ void k_write_tail(uint32_t* __restrict__ occ_off, uint32_t n_kept, const Counters* __restrict__ ctr,
                             const unsigned long long* __restrict__ dn) {
    // (occ_off holds n_kept + 1 entries: a unique count past that is never written)
    if (threadIdx.x == 0 && ctr->n_unique <= n_kept) occ_off[ctr->n_unique] = dn ? (uint32_t)*dn : n_kept;
}

hipError_t launch_write_tail(uint32_t* d_occ_off, uint32_t n_kept, const Counters* d_ctr, hipStream_t s,
                             const unsigned long long* d_n) {
    DBI_LAUNCH(k_write_tail, dim3(1), dim3(64), 0, s, d_occ_off, n_kept, d_ctr, d_n);
    return hipGetLastError();
}

// STREAM-like copy (dbi_hbm_copy_bandwidth): the measured HBM ceiling printed
// next to the 8 TB/s peak.  One-shot grid, four 16-B streaming loads in flight
// per thread (tools/copy_probe.hip: 6.4 TB/s; a grid-stride loop 4.8, default
// cache policy 5.9, eight per thread 4.4).
constexpr uint32_t COPY_ITEMS = 4;
__global__ void __launch_bounds__(256) k_hbm_copy(const uint4* __restrict__ in, uint4* __restrict__ out, uint64_t n) {
    const uint64_t base = (uint64_t)blockIdx.x * 256u * COPY_ITEMS + threadIdx.x;
    uint4 v[COPY_ITEMS];
#pragma unroll
    for (uint32_t k = 0; k < COPY_ITEMS; ++k) {
        const uint64_t i = base + (uint64_t)k * 256u;
        if (i < n) v[k] = ld16<true>(in + i);
    }
#pragma unroll
    for (uint32_t k = 0; k < COPY_ITEMS; ++k) {
        const uint64_t i = base + (uint64_t)k * 256u;
        if (i < n) st16<true>(out + i, v[k]);
    }
}

hipError_t launch_hbm_copy(const void* d_in, void* d_out, uint64_t n16, hipStream_t s) {
    const uint64_t blocks = (n16 + 256u * COPY_ITEMS - 1) / (256u * COPY_ITEMS);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    DBI_LAUNCH(k_hbm_copy, dim3((uint32_t)blocks), dim3(256), 0, s, reinterpret_cast<const uint4*>(d_in),
               reinterpret_cast<uint4*>(d_out), n16);
    return hipGetLastError();
}

// gather per-unique data for arbitrary ids (dbi_peptides)
__global__ void k_gather(const uint64_t* __restrict__ ids, uint64_t n, const double* __restrict__ umass,
                         const uint32_t* __restrict__ upid, const uint32_t* __restrict__ uoff,
                         const uint32_t* __restrict__ ulen, const uint32_t* __restrict__ occ_off,
                         double* __restrict__ o_mass, uint32_t* __restrict__ o_pid, uint32_t* __restrict__ o_off,
                         uint32_t* __restrict__ o_len, uint64_t* __restrict__ o_b, uint64_t* __restrict__ o_e) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t u = ids[i];
    o_mass[i] = umass[u];
    o_pid[i] = upid[u];
    o_off[i] = uoff[u];
    o_len[i] = ulen[u];
    o_b[i] = occ_off[u];
    o_e[i] = occ_off[u + 1];
}

hipError_t launch_gather(const uint64_t* d_ids, uint64_t n, const double* d_umass, const uint32_t* d_upid,
                         const uint32_t* d_uoff, const uint32_t* d_ulen, const uint32_t* d_occ_off,
                         double* o_mass, uint32_t* o_pid, uint32_t* o_off, uint32_t* o_len, uint64_t* o_b,
                         uint64_t* o_e, hipStream_t s) {
    if (n == 0) return hipSuccess;
    DBI_LAUNCH(k_gather, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d_ids, n, d_umass, d_upid,
                       d_uoff, d_ulen, d_occ_off, o_mass, o_pid, o_off, o_len, o_b, o_e);
    return hipGetLastError();
}

__global__ void k_write_keys(const double* __restrict__ umass, uint32_t n, int32_t factor,
                             const uint32_t* __restrict__ pos, int32_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t k = java_d2i(umass[i] * (double)factor);
    if (i == 0 || java_d2i(umass[i - 1] * (double)factor) != k) keys[pos[i]] = k;
}

hipError_t launch_write_keys(const double* d_umass, uint32_t n_unique, int32_t factor, const uint32_t* d_pos,
                             int32_t* d_keys, hipStream_t s) {
    if (n_unique == 0) return hipSuccess;
    DBI_LAUNCH(k_write_keys, dim3((n_unique + 255) / 256), dim3(256), 0, s, d_umass, n_unique, factor,
                       d_pos, d_keys);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// query: getSequences(m, tol) (SQLiteMult:315-350 + IndexMerge:146-217,386-481)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lower_bound_d(const double* __restrict__ a, uint32_t n, double x) {
    uint32_t lo = 0, hi = n;  // first i with a[i] >= x
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t upper_bound_d(const double* __restrict__ a, uint32_t n, double x) {
    uint32_t lo = 0, hi = n;  // first i with a[i] > x
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// [lo, hi) variants: the result lies in [lo, hi]
__device__ __forceinline__ uint32_t lower_bound_in(const double* __restrict__ a, uint32_t lo, uint32_t hi, double x) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t upper_bound_in(const double* __restrict__ a, uint32_t lo, uint32_t hi, double x) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Query directory over the unique masses: bucket(m) = clamp((m - lo) * scale)
// is monotone in m, so dir[b] = first unique with bucket >= b brackets every
// bound of a mass in bucket b: lower/upper_bound(x) lie in [dir[b], dir[b+1]].
// The binary search then runs over ~4 uniques instead of all of them.
__device__ __forceinline__ uint32_t qdir_bucket(const QueryDir& qd, double m) {
    const double t = (m - qd.lo) * qd.scale;
    if (!(t > 0.0)) return 0u;
    if (t >= (double)(qd.nb - 1)) return qd.nb - 1;
    return (uint32_t)t;
}

__global__ void k_qdir_params(const double* __restrict__ umass, uint32_t nu, uint32_t nb, QueryDir* qd) {
    if (threadIdx.x != 0) return;
    const double lo = nu ? umass[0] : 0.0, hi = nu ? umass[nu - 1] : 0.0;
    qd->lo = lo;
    qd->scale = hi > lo ? (double)nb / (hi - lo) : 0.0;
    qd->nb = nb;
}

__global__ void k_qdir_fill(const double* __restrict__ umass, uint32_t nu, const QueryDir* __restrict__ qdp,
                            uint32_t* __restrict__ dir) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nu) return;
    const QueryDir qd = *qdp;
    const uint32_t bi = i < nu ? qdir_bucket(qd, umass[i]) : qd.nb;  // past the last unique: every bucket left
    const uint32_t b0 = i == 0 ? 0u : qdir_bucket(qd, umass[i - 1]) + 1;
    for (uint32_t k = b0; k <= bi; ++k) dir[k] = i;
}

hipError_t launch_qdir(const double* d_umass, uint32_t nu, uint32_t nb, QueryDir* d_qd, uint32_t* d_dir,
                       hipStream_t s) {
    DBI_LAUNCH(k_qdir_params, dim3(1), dim3(64), 0, s, d_umass, nu, nb, d_qd);
    DBI_LAUNCH(k_qdir_fill, dim3((nu + 1 + 255) / 256), dim3(256), 0, s, d_umass, nu, d_qd, d_dir);
    return hipGetLastError();
}

// first i with key(a[i]) > k   (key monotone in mass)
__device__ __forceinline__ uint32_t key_upper(const double* __restrict__ a, uint32_t n, int32_t factor, int32_t k) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (java_d2i(a[mid] * (double)factor) <= k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void k_query(DevParams dp, int32_t factor, const double* __restrict__ umass, uint32_t nu,
                        const double* __restrict__ qm, const double* __restrict__ qt, uint64_t nq,
                        uint64_t* __restrict__ first, uint64_t* __restrict__ count,
                        const QueryDir* __restrict__ qdp, const uint32_t* __restrict__ dir) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const QueryDir qd = *qdp;
    auto lower_bound_d = [&](const double* a, uint32_t n, double x) {
        const uint32_t b = qdir_bucket(qd, x);
        return lower_bound_in(a, dir[b], dir[b + 1], x);
    };
    auto upper_bound_d = [&](const double* a, uint32_t n, double x) {
        const uint32_t b = qdir_bucket(qd, x);
        return upper_bound_in(a, dir[b], dir[b + 1], x);
    };
    const double precMass = qm[i], tol = qt[i];
    double lo = precMass - tol;
    if (lo < 0) lo = 0;
    const double hi = precMass + tol;
    const int b0 = java_d2i(lo) / dp.br, b1 = java_d2i(hi) / dp.br;
    uint64_t f = 0, c = 0;
    if (!dp.buckets) {
        // MassRangeFilteringIndex.filterSequence (:90-108): minMass <= m <= maxMass,
        // no buckets; a NaN bound includes nothing
        if (lo == lo && hi == hi) {
            const uint32_t a = lower_bound_d(umass, nu, lo);
            const uint32_t e = upper_bound_d(umass, nu, hi);
            if (e > a) { f = a; c = e - a; }
        }
    } else if (!(b0 > dp.nb - 1 || b1 > dp.nb - 1)) {
        if (lo != lo || hi != hi) {
            // NaN bounds: rows BETWEEN (int)NaN=0 AND 0, and no mass test rejects
            // (comparisons with NaN are false) -> every unique with key 0.
            c = key_upper(umass, nu, factor, 0);
        } else {
            const uint32_t a = lower_bound_d(umass, nu, lo);
            const uint32_t e = upper_bound_d(umass, nu, hi);
            if (e > a) { f = a; c = e - a; }
        }
    }
    first[i] = f;
    count[i] = c;
}

hipError_t launch_query(const DevParams& dp, int32_t factor, const double* d_umass, uint32_t n_unique,
                        const double* d_qmass, const double* d_qtol, uint64_t nq, uint64_t* d_first,
                        uint64_t* d_count, const QueryDir* d_qd, const uint32_t* d_dir, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    DBI_LAUNCH(k_query, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, s, dp, factor, d_umass,
                       n_unique, d_qmass, d_qtol, nq, d_first, d_count, d_qd, d_dir);
    return hipGetLastError();
}

// unique-id range [out[0], out[1]) of keys in [klo, khi]
__global__ void k_key_range(const double* __restrict__ umass, uint32_t nu, int32_t factor, int32_t klo,
                            int32_t khi, uint64_t* out) {
    if (threadIdx.x != 0) return;
    out[0] = klo == (-2147483647 - 1) ? 0u : key_upper(umass, nu, factor, klo - 1);
    out[1] = key_upper(umass, nu, factor, khi);
}

hipError_t launch_key_range(const double* d_umass, uint32_t n_unique, int32_t factor, int32_t klo,
                            int32_t khi, uint64_t* d_out2, hipStream_t s) {
    DBI_LAUNCH(k_key_range, dim3(1), dim3(64), 0, s, d_umass, n_unique, factor, klo, khi, d_out2);
    return hipGetLastError();
}

__global__ void k_expand_csr(const uint64_t* __restrict__ first, const uint64_t* __restrict__ count,
                             const uint64_t* __restrict__ row, uint64_t nq, uint64_t* __restrict__ ids) {
    const uint64_t q = blockIdx.x;
    if (q >= nq) return;
    const uint64_t f = first[q], c = count[q], o = row[q];
    for (uint64_t k = threadIdx.x; k < c; k += blockDim.x) ids[o + k] = f + k;
}

hipError_t launch_expand_csr(const uint64_t* d_first, const uint64_t* d_count, const uint64_t* d_row,
                             uint64_t nq, uint64_t* d_ids, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    DBI_LAUNCH(k_expand_csr, dim3((uint32_t)nq), dim3(64), 0, s, d_first, d_count, d_row, nq, d_ids);
    return hipGetLastError();
}

// ---- hit materialisation (dbi_query_hits_device) ---------------------------------
// The hits of one window are the consecutive unique ids [first, first+count)
// (IndexMerge.parseAddPeptideInfo :386-481 walks them in mass order), and the
// proteins of those peptides (the row blob's protein-id lists, :446-470) are
// the consecutive occurrence slots [occ_off[first], occ_off[first+count]).
// Per query: hits, proteins of its hits; per hit: its unique id and where its
// protein list starts inside the query's.
__global__ void k_hits_count(const uint64_t* __restrict__ first, const uint64_t* __restrict__ count,
                             const uint32_t* __restrict__ occ_off, uint64_t nq, uint32_t* __restrict__ nh,
                             uint32_t* __restrict__ no) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint64_t f = first[i], c = count[i];
    nh[i] = (uint32_t)c;
    no[i] = c ? occ_off[f + c] - occ_off[f] : 0u;
}

// exclusive scans of two u32 arrays into u64 offsets (+ totals), the same
// three phases as launch_scan_u32
__global__ void __launch_bounds__(SCAN_THREADS)
k_scan2_reduce(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint64_t n,
               unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long tmp[SCAN_THREADS / 64 + 1];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_CHUNK;
    unsigned long long va = 0, vb = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const uint64_t i = base + (uint64_t)k * SCAN_THREADS + threadIdx.x;
        if (i < n) { va += a[i]; vb += b[i]; }
    }
    const unsigned long long ta = block_sum<SCAN_THREADS, unsigned long long>(va, tmp);
    __syncthreads();
    const unsigned long long tb = block_sum<SCAN_THREADS, unsigned long long>(vb, tmp);
    if (threadIdx.x == 0) {
        sums[2 * blockIdx.x] = ta;
        sums[2 * blockIdx.x + 1] = tb;
    }
}

// one block: exclusive scan of the nb block sums (pairs) in place, totals to tot[0..1]
__global__ void __launch_bounds__(SCAN_THREADS)
k_scan2_single(unsigned long long* __restrict__ sums, uint64_t nb, unsigned long long* __restrict__ tot) {
    __shared__ unsigned long long tmp[SCAN_THREADS / 64 + 1];
    for (int h = 0; h < 2; ++h) {
        unsigned long long carry = 0;
        for (uint64_t base = 0; base < nb; base += SCAN_THREADS) {
            const uint64_t i = base + threadIdx.x;
            const unsigned long long v = i < nb ? sums[2 * i + h] : 0ull;
            unsigned long long t;
            const unsigned long long e = block_excl_scan<SCAN_THREADS, unsigned long long>(v, tmp, t);
            if (i < nb) sums[2 * i + h] = carry + e;
            carry += t;
            __syncthreads();
        }
        if (threadIdx.x == 0) tot[h] = carry;
    }
}

__global__ void __launch_bounds__(SCAN_THREADS)
k_scan2_down(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint64_t n,
             const unsigned long long* __restrict__ sums, const unsigned long long* __restrict__ tot,
             uint64_t* __restrict__ oa, uint64_t* __restrict__ ob) {
    __shared__ unsigned long long tmp[SCAN_THREADS / 64 + 1];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_CHUNK;
    uint32_t va[SCAN_ITEMS], vb[SCAN_ITEMS];
    unsigned long long la = 0, lb = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const uint64_t i = base + (uint64_t)threadIdx.x * SCAN_ITEMS + k;
        va[k] = i < n ? a[i] : 0u;
        vb[k] = i < n ? b[i] : 0u;
        la += va[k];
        lb += vb[k];
    }
    unsigned long long t;
    unsigned long long ra = block_excl_scan<SCAN_THREADS, unsigned long long>(la, tmp, t) + sums[2 * blockIdx.x];
    __syncthreads();
    unsigned long long rb = block_excl_scan<SCAN_THREADS, unsigned long long>(lb, tmp, t) + sums[2 * blockIdx.x + 1];
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const uint64_t i = base + (uint64_t)threadIdx.x * SCAN_ITEMS + k;
        if (i < n) { oa[i] = ra; ob[i] = rb; }
        ra += va[k];
        rb += vb[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { oa[n] = tot[0]; ob[n] = tot[1]; }
}

size_t scan2_tmp_elems(uint64_t n) { return 2 * (size_t)((n + SCAN_CHUNK - 1) / SCAN_CHUNK) + 2; }

hipError_t launch_hits_offsets(const uint64_t* d_first, const uint64_t* d_count, const uint32_t* d_occ_off,
                               uint64_t nq, uint32_t* d_nh, uint32_t* d_no, unsigned long long* d_sums,
                               uint64_t* d_row, uint64_t* d_occ_row, unsigned long long* d_tot, hipStream_t s) {
    const uint64_t nb = std::max<uint64_t>((nq + SCAN_CHUNK - 1) / SCAN_CHUNK, 1);
    DBI_LAUNCH(k_hits_count, dim3((uint32_t)((nq + 255) / 256 + 1)), dim3(256), 0, s, d_first, d_count, d_occ_off,
               nq, d_nh, d_no);
    DBI_LAUNCH(k_scan2_reduce, dim3((uint32_t)nb), dim3(SCAN_THREADS), 0, s, d_nh, d_no, nq, d_sums);
    DBI_LAUNCH(k_scan2_single, dim3(1), dim3(SCAN_THREADS), 0, s, d_sums, nb, d_tot);
    DBI_LAUNCH(k_scan2_down, dim3((uint32_t)nb), dim3(SCAN_THREADS), 0, s, d_nh, d_no, nq, d_sums, d_tot, d_row,
               d_occ_row);
    return hipGetLastError();
}

// One block per query (grid-stride): the ids of its hits, each hit's protein
// list start relative to the query's, and the protein ids themselves — all
// three contiguous runs, written with consecutive lanes on consecutive words.
constexpr uint32_t HITS_THREADS = 256;
__global__ void __launch_bounds__(HITS_THREADS)
k_hits_expand(const uint64_t* __restrict__ first, const uint64_t* __restrict__ count,
              const uint64_t* __restrict__ row, const uint64_t* __restrict__ occ_row,
              const uint32_t* __restrict__ occ_off, const uint32_t* __restrict__ occ_pid, uint64_t nq,
              uint32_t* __restrict__ ids, uint32_t* __restrict__ hit_occ, uint32_t* __restrict__ prot) {
    for (uint64_t q = blockIdx.x; q < nq; q += gridDim.x) {
        const uint64_t c = count[q];
        if (c == 0) continue;
        const uint32_t f = (uint32_t)first[q];
        const uint64_t r = row[q], orow = occ_row[q];
        const uint32_t o0 = occ_off[f], o1 = occ_off[f + c];
        for (uint32_t k = threadIdx.x; k < c; k += HITS_THREADS) {
            ids[r + k] = f + k;
            hit_occ[r + k] = occ_off[f + k] - o0;
        }
        for (uint32_t k = threadIdx.x; k < o1 - o0; k += HITS_THREADS) prot[orow + k] = occ_pid[o0 + k];
    }
}

hipError_t launch_hits_expand(const uint64_t* d_first, const uint64_t* d_count, const uint64_t* d_row,
                              const uint64_t* d_occ_row, const uint32_t* d_occ_off, const uint32_t* d_occ_pid,
                              uint64_t nq, uint32_t* d_ids, uint32_t* d_hit_occ, uint32_t* d_prot, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    const uint32_t g = (uint32_t)std::min<uint64_t>(nq, 256u * 64u);  // 64 blocks per CU, grid-stride
    DBI_LAUNCH(k_hits_expand, dim3(g), dim3(HITS_THREADS), 0, s, d_first, d_count, d_row, d_occ_row, d_occ_off,
               d_occ_pid, nq, d_ids, d_hit_occ, d_prot);
    return hipGetLastError();
}

// host-supplied occurrences -> records (DBIndexStore.addSequence path; the
// host checked 1 <= mass < 65536 and that every occurrence lies in its protein)
__global__ void k_occ_to_recs(const double* __restrict__ mass, const uint32_t* __restrict__ pid,
                              const uint32_t* __restrict__ off, const uint32_t* __restrict__ len,
                              const uint32_t* __restrict__ poff, const uint8_t* __restrict__ res, uint64_t n,
                              uint64_t n_prot, Rec* __restrict__ out, Counters* __restrict__ ctr) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t W = rec_width(ctr->max_plen);
    if (i == 0 && !rec_layout_ok(W, n_prot)) atomicOr(&ctr->err, ERR_LAYOUT);
    if (i >= n) return;
    const uint32_t p = pid[i], o = off[i], l = len[i];
    const uint32_t tag = peptide_tag_of(res + poff[p] + o, l);
    Rec r;
    r.q0 = rec_q0(mass[i], tag);
    r.q1 = rec_q1(tag, rec_loc(p, o, W), l);
    out[i] = r;
}

hipError_t launch_occ_to_recs(const double* d_mass, const uint32_t* d_pid, const uint32_t* d_off,
                              const uint32_t* d_len, const uint32_t* d_poff, const uint8_t* d_res, uint64_t n,
                              uint64_t n_prot, Rec* d_out, Counters* d_ctr, hipStream_t s) {
    if (n == 0) return hipSuccess;
    DBI_LAUNCH(k_occ_to_recs, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d_mass, d_pid, d_off,
                       d_len, d_poff, d_res, n, n_prot, d_out, d_ctr);
    return hipGetLastError();
}

__global__ void k_off64_to_32(const uint64_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n,
                              Counters* __restrict__ ctr) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint32_t)in[i];
    if (ctr && blockIdx.x == 0)  // a build's counters back to zero (dbi_build_device: a memset fewer)
        for (uint32_t k = threadIdx.x; k < sizeof(Counters) / 4; k += blockDim.x) reinterpret_cast<uint32_t*>(ctr)[k] = 0;
}

hipError_t launch_off64_to_32(const uint64_t* d_in, uint32_t* d_out, uint64_t n, hipStream_t s, Counters* d_ctr) {
    if (n == 0) return d_ctr ? hipMemsetAsync(d_ctr, 0, sizeof(Counters), s) : hipSuccess;
    DBI_LAUNCH(k_off64_to_32, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d_in, d_out, n, d_ctr);
    return hipGetLastError();
}

}  // namespace dbi

namespace dbi {

// ---------------------------------------------------------------------------
// sharded build helpers (dbi_shard.hip)
// ---------------------------------------------------------------------------
__global__ void k_sample_masses(const Rec* __restrict__ recs, uint64_t n, uint32_t ns, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const uint64_t j = (uint64_t)(((unsigned __int128)i * n) / ns);
    const uint64_t q0 = recs[j].q0;
    out[i] = q0 == REC_SENTINEL ? __builtin_nan("") : q0_mass(q0);
}

hipError_t launch_sample_masses(const Rec* d_recs, uint64_t n, uint32_t ns, double* d_out, hipStream_t s) {
    if (ns == 0) return hipSuccess;
    if (n == 0) return hipMemsetAsync(d_out, 0xFF, sizeof(double) * ns, s);  // all NaN
    DBI_LAUNCH(k_sample_masses, dim3((ns + 255) / 256), dim3(256), 0, s, d_recs, n, ns, d_out);
    return hipGetLastError();
}

// clamped into [0, hi]: a device-sized shard digest rebases by the residue
// range of the last build, which offsets rewritten since may leave (the build
// is flagged and redone; meanwhile nothing reads outside the residues)
__global__ void k_off_rebase(const uint64_t* __restrict__ in, uint64_t base, uint64_t hi, uint32_t* __restrict__ out,
                             uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] <= base ? 0u : (uint32_t)min(in[i] - base, hi);
}

hipError_t launch_off_rebase(const uint64_t* d_in, uint64_t base, uint64_t hi, uint32_t* d_out, uint64_t n,
                             hipStream_t s) {
    if (n == 0) return hipSuccess;
    DBI_LAUNCH(k_off_rebase, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d_in, base, hi, d_out, n);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) k_max_plen(const uint32_t* __restrict__ poff, uint32_t n_prot,
                                                  Counters* __restrict__ ctr) {
    uint32_t m = 0;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_prot; p += gridDim.x * blockDim.x)
        m = max(m, poff[p + 1] - poff[p]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    __shared__ uint32_t s_max[4];
    if (lane_id() == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&ctr->max_plen, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
}

hipError_t launch_max_plen(const uint32_t* d_poff, uint32_t n_prot, Counters* d_ctr, hipStream_t s) {
    if (n_prot == 0) return hipSuccess;
    const uint32_t g = std::min<uint32_t>((n_prot + 255) / 256, 1024u);
    DBI_LAUNCH(k_max_plen, dim3(g), dim3(256), 0, s, d_poff, n_prot, d_ctr);
    return hipGetLastError();
}

}  // namespace dbi

namespace dbi {

// ---------------------------------------------------------------------------
// sharded queries: route windows to key owners, answer, fold back
// (getSequences(m, tol), DBIndexStoreSQLiteMult.java:315-350)
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool query_window(double m, double t, int32_t nb, int32_t br, double& lo, double& hi) {
    lo = m - t;
    if (lo < 0) lo = 0;
    hi = m + t;
    const int b0 = java_d2i(lo) / br, b1 = java_d2i(hi) / br;
    return !(b0 > nb - 1 || b1 > nb - 1);
}

__device__ __forceinline__ uint32_t owner_of_key(const RouteMap& rm, int32_t k) {
    uint32_t d = 0;
    for (uint32_t j = 0; j + 1 < rm.nshards; ++j) d += k >= rm.split[j] ? 1u : 0u;
    return d;
}

__device__ __forceinline__ bool route_span(const RouteMap& rm, double m, double t, uint32_t& o0, uint32_t& o1) {
    double lo, hi;
    if (!query_window(m, t, rm.nb, rm.br, lo, hi)) return false;
    o0 = owner_of_key(rm, java_d2i(lo * (double)rm.factor));
    o1 = owner_of_key(rm, java_d2i(hi * (double)rm.factor));
    if (o1 < o0) o1 = o0;  // NaN bounds: key 0 on both sides
    return true;
}

__global__ void k_qroute_count(const double* __restrict__ qm, const double* __restrict__ qt, uint64_t nq, RouteMap rm,
                               uint32_t* __restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    uint32_t o0 = 0, o1 = 0;
    cnt[i] = route_span(rm, qm[i], qt[i], o0, o1) ? o1 - o0 + 1 : 0u;
}

hipError_t launch_qroute_count(const double* d_qm, const double* d_qt, uint64_t nq, const RouteMap& rm,
                               uint32_t* d_cnt, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    DBI_LAUNCH(k_qroute_count, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, s, d_qm, d_qt, nq, rm, d_cnt);
    return hipGetLastError();
}

__global__ void k_qroute_emit(const double* __restrict__ qm, const double* __restrict__ qt, uint64_t nq, RouteMap rm,
                              const uint32_t* __restrict__ offs, Rec* __restrict__ pairs) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    uint32_t o0 = 0, o1 = 0;
    if (!route_span(rm, qm[i], qt[i], o0, o1)) return;
    Rec* __restrict__ out = pairs + offs[i];
    for (uint32_t o = o0; o <= o1; ++o) {
        Rec r;
        r.q0 = o;
        r.q1 = i;
        out[o - o0] = r;
    }
}

hipError_t launch_qroute_emit(const double* d_qm, const double* d_qt, uint64_t nq, const RouteMap& rm,
                              const uint32_t* d_offs, Rec* d_pairs, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    DBI_LAUNCH(k_qroute_emit, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, s, d_qm, d_qt, nq, rm, d_offs,
               d_pairs);
    return hipGetLastError();
}

__global__ void k_qpack(const Rec* __restrict__ pairs, uint64_t np, const double* __restrict__ qm,
                        const double* __restrict__ qt, Rec* __restrict__ out) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const uint64_t i = pairs[p].q1;
    Rec r;
    r.q0 = (uint64_t)__double_as_longlong(qm[i]);
    r.q1 = (uint64_t)__double_as_longlong(qt[i]);
    out[p] = r;
}

hipError_t launch_qpack(const Rec* d_pairs, uint64_t np, const double* d_qm, const double* d_qt, Rec* d_out,
                        hipStream_t s) {
    if (np == 0) return hipSuccess;
    DBI_LAUNCH(k_qpack, dim3((uint32_t)((np + 255) / 256)), dim3(256), 0, s, d_pairs, np, d_qm, d_qt, d_out);
    return hipGetLastError();
}

__global__ void k_query_pairs(DevParams dp, int32_t factor, const double* __restrict__ umass, uint32_t nu,
                              const Rec* __restrict__ in, uint64_t n, uint64_t base, Rec* __restrict__ out,
                              const QueryDir* __restrict__ qdp, const uint32_t* __restrict__ dir) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const QueryDir qd = *qdp;
    auto lower_bound_d = [&](const double* a, uint32_t, double x) {
        const uint32_t b = qdir_bucket(qd, x);
        return lower_bound_in(a, dir[b], dir[b + 1], x);
    };
    auto upper_bound_d = [&](const double* a, uint32_t, double x) {
        const uint32_t b = qdir_bucket(qd, x);
        return upper_bound_in(a, dir[b], dir[b + 1], x);
    };
    const Rec q = in[i];
    const double precMass = __longlong_as_double((long long)q.q0), tol = __longlong_as_double((long long)q.q1);
    double lo, hi;
    uint64_t f = 0, c = 0;
    if (query_window(precMass, tol, dp.nb, dp.br, lo, hi)) {
        if (lo != lo || hi != hi) {
            c = key_upper(umass, nu, factor, 0);  // k_query: NaN bounds select key 0
        } else {
            const uint32_t a = lower_bound_d(umass, nu, lo);
            const uint32_t e = upper_bound_d(umass, nu, hi);
            if (e > a) { f = a; c = e - a; }
        }
    }
    Rec r;
    r.q0 = c ? base + f : ~0ull;
    r.q1 = c;
    out[i] = r;
}

hipError_t launch_query_pairs(const DevParams& dp, int32_t factor, const double* d_umass, uint32_t n_unique,
                              const Rec* d_in, uint64_t n, uint64_t base, Rec* d_out, const QueryDir* d_qd,
                              const uint32_t* d_dir, hipStream_t s) {
    if (n == 0) return hipSuccess;
    DBI_LAUNCH(k_query_pairs, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, dp, factor, d_umass, n_unique,
               d_in, n, base, d_out, d_qd, d_dir);
    return hipGetLastError();
}

__global__ void k_qcombine_init(uint64_t* __restrict__ first, uint64_t* __restrict__ count, uint64_t nq) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    first[i] = ~0ull;
    count[i] = 0;
}

// a window's owners are consecutive and their id ranges adjacent in the
// concatenated table: first = min over owners that hit, count = sum
__global__ void k_qcombine(const Rec* __restrict__ pairs, const Rec* __restrict__ res, uint64_t np,
                           unsigned long long* __restrict__ first, unsigned long long* __restrict__ count) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const Rec r = res[p];
    if (r.q1 == 0) return;
    const uint64_t q = pairs[p].q1;
    atomicAdd(&count[q], (unsigned long long)r.q1);
    atomicMin(&first[q], (unsigned long long)r.q0);
}

__global__ void k_qcombine_fix(uint64_t* __restrict__ first, uint64_t nq) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq && first[i] == ~0ull) first[i] = 0;
}

hipError_t launch_qcombine(const Rec* d_pairs, const Rec* d_res, uint64_t np, uint64_t* d_first, uint64_t* d_count,
                           uint64_t nq, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    const dim3 gq((uint32_t)((nq + 255) / 256));
    DBI_LAUNCH(k_qcombine_init, gq, dim3(256), 0, s, d_first, d_count, nq);
    if (np)
        DBI_LAUNCH(k_qcombine, dim3((uint32_t)((np + 255) / 256)), dim3(256), 0, s, d_pairs, d_res, np,
                   (unsigned long long*)d_first, (unsigned long long*)d_count);
    DBI_LAUNCH(k_qcombine_fix, gq, dim3(256), 0, s, d_first, nq);
    return hipGetLastError();
}

}  // namespace dbi

namespace dbi {

// ---------------------------------------------------------------------------
// 5c. chunks above BIG_CAP: MSD split on the 72-bit (mass, tag) key
// ---------------------------------------------------------------------------
// Such chunks are equal-mass spikes: thousands of isobaric peptides with
// bit-identical fp64 masses (semi-tryptic SwissProt: tens of thousands).  Their
// sorted order is by (q0, q1) = (mass, tag, first appearance), so a split on
// the top varying bits of X = (q0, q1 >> 56) — the tag splits an equal-mass
// spike 65536 ways — gives ordered sub-buckets, and an equal-(mass, tag) group
// (the only place dedup compares strings) never straddles two of them.
// Adjacent small sub-buckets are packed into leaves of <= CHUNK_CAP records,
// sorted in LDS like any chunk; their unique counts add into the chunk's.
// A segment is uint4 {lo, n, chunk, buf}: records [lo, lo+n) in `in` (buf 0)
// or `out` (buf 1).
struct GiantLists {
    uint4* work[GIANT_PASSES + 1];
    uint4* leaf_small;
    uint4* leaf_big;
    uint4* fallback;
    uint32_t cap;
};

size_t giant_seg_cap(uint64_t n) { return (size_t)(n / 64 + 4096); }

__device__ __forceinline__ unsigned __int128 key72(const Rec& r) {
    return ((unsigned __int128)r.q0 << 8) | (unsigned __int128)(r.q1 >> 56);
}

__device__ __forceinline__ void seg_push(uint4* list, unsigned int* cnt, uint32_t cap, uint4 seg,
                                         Counters* ctr) {
    const unsigned int i = atomicAdd(cnt, 1u);
    if (i < cap) list[i] = seg;
    else atomicOr(&ctr->err, ERR_SEGS);
}

__global__ void k_giant_init(const uint32_t* __restrict__ giant_list, const uint32_t* __restrict__ chunk_lo,
                             uint32_t* __restrict__ ucount, GiantLists gl, Counters* __restrict__ ctr) {
    const uint32_t n = ctr->n_giant;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const uint32_t c = giant_list[j];
        const uint32_t a = chunk_lo[c];
        ucount[c] = 0;
        if (j < gl.cap) gl.work[0][j] = make_uint4(a, chunk_lo[c + 1] - a, c, 0u);
        else atomicOr(&ctr->err, ERR_SEGS);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctr->n_seg[0] = min(n, gl.cap);
}

constexpr int SPLIT_THREADS = 1024;
constexpr uint32_t SPLIT_ITEMS = 4;  // records per thread in a scatter tile

__global__ void __launch_bounds__(SPLIT_THREADS)
k_giant_split(Rec* in, Rec* out, GiantLists gl, int pass, Counters* __restrict__ ctr) {
    __shared__ uint32_t cnt[256];
    __shared__ uint32_t cur[256];
    __shared__ uint32_t wcnt[SPLIT_THREADS / 64][256];  // per-wave digit counts of one scatter tile
    for (uint32_t x = threadIdx.x; x < (SPLIT_THREADS / 64) * 256; x += SPLIT_THREADS) (&wcnt[0][0])[x] = 0;
    __shared__ unsigned long long s_lo0[SPLIT_THREADS / 64], s_hi0[SPLIT_THREADS / 64];
    __shared__ uint32_t s_lo1[SPLIT_THREADS / 64], s_hi1[SPLIT_THREADS / 64];
    __shared__ uint32_t s_shift, s_same;
    __shared__ uint4 s_ent[256];  // a segment's new list entries, their list (0 small leaf, 1 big leaf,
    __shared__ uint8_t s_kind[256];  // 2 next pass, 3 fallback) and rank in it
    __shared__ uint32_t s_rank[256], s_base[4], s_ne;
    const uint32_t nseg = ctr->n_seg[pass];
    const bool last = pass + 1 == GIANT_PASSES;
    for (uint32_t j = blockIdx.x; j < nseg; j += gridDim.x) {
        const uint4 seg = gl.work[pass][j];
        const uint32_t lo = seg.x, n = seg.y;
        const Rec* __restrict__ from = seg.w ? out : in;
        Rec* __restrict__ to = seg.w ? in : out;
        // min / max of the 72-bit key over the segment
        unsigned __int128 kmin = ~(unsigned __int128)0, kmax = 0;
        for (uint32_t t0 = 0; t0 < n; t0 += SPLIT_THREADS * SPLIT_ITEMS) {
            Rec r[SPLIT_ITEMS];  // all loads of a round in flight together
#pragma unroll
            for (uint32_t k = 0; k < SPLIT_ITEMS; ++k) {
                const uint32_t i = min(t0 + k * SPLIT_THREADS + threadIdx.x, n - 1);  // (a repeat is harmless)
                r[k] = from[lo + i];
            }
#pragma unroll
            for (uint32_t k = 0; k < SPLIT_ITEMS; ++k) {
                const unsigned __int128 x = key72(r[k]);
                kmin = x < kmin ? x : kmin;
                kmax = x > kmax ? x : kmax;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const uint64_t a0 = (uint64_t)(kmin >> 8), b0 = (uint64_t)(kmax >> 8);
            const uint32_t a1 = (uint32_t)(kmin & 0xFF), b1 = (uint32_t)(kmax & 0xFF);
            const uint64_t o0 = (uint64_t)__shfl_xor((long long)a0, d, 64), p0 = (uint64_t)__shfl_xor((long long)b0, d, 64);
            const uint32_t o1 = (uint32_t)__shfl_xor((int)a1, d, 64), p1 = (uint32_t)__shfl_xor((int)b1, d, 64);
            const unsigned __int128 om = ((unsigned __int128)o0 << 8) | o1, pm = ((unsigned __int128)p0 << 8) | p1;
            kmin = om < kmin ? om : kmin;
            kmax = pm > kmax ? pm : kmax;
        }
        const uint32_t w = threadIdx.x >> 6;
        if (lane_id() == 0) {
            s_lo0[w] = (uint64_t)(kmin >> 8); s_lo1[w] = (uint32_t)(kmin & 0xFF);
            s_hi0[w] = (uint64_t)(kmax >> 8); s_hi1[w] = (uint32_t)(kmax & 0xFF);
        }
        if (threadIdx.x < 256) cnt[threadIdx.x] = 0;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned __int128 a = ~(unsigned __int128)0, b = 0;
            for (int q = 0; q < SPLIT_THREADS / 64; ++q) {
                const unsigned __int128 x = ((unsigned __int128)s_lo0[q] << 8) | s_lo1[q];
                const unsigned __int128 y = ((unsigned __int128)s_hi0[q] << 8) | s_hi1[q];
                a = x < a ? x : a;
                b = y > b ? y : b;
            }
            const unsigned __int128 diff = a ^ b;
            uint32_t v = 0;  // varying bits
            if (diff >> 64) v = 128 - __clzll((unsigned long long)(diff >> 64));
            else if (diff) v = 64 - __clzll((unsigned long long)diff);
            s_same = diff == 0;
            s_shift = v > 8 ? v - 8 : 0;
        }
        __syncthreads();
        if (s_same) {
            // one (mass, tag) key: strings decide, no key bits left to split on
            if (threadIdx.x == 0) seg_push(gl.fallback, &ctr->n_fallback, gl.cap, seg, ctr);
            __syncthreads();
            continue;
        }
        const uint32_t sh = s_shift;
        // digit counts: one LDS add per distinct digit of a wave (a spike's
        // records share a few digits: per-record adds serialise on them)
        for (uint32_t t0 = 0; t0 < n; t0 += SPLIT_THREADS * SPLIT_ITEMS) {
            Rec r[SPLIT_ITEMS];
#pragma unroll
            for (uint32_t k = 0; k < SPLIT_ITEMS; ++k) {
                const uint32_t i = t0 + k * SPLIT_THREADS + threadIdx.x;
                r[k] = i < n ? from[lo + i] : Rec{0, 0};
            }
#pragma unroll
            for (uint32_t k = 0; k < SPLIT_ITEMS; ++k) {
                const bool valid = t0 + k * SPLIT_THREADS + threadIdx.x < n;
                const uint32_t d = valid ? (uint32_t)(key72(r[k]) >> sh) & 0xFFu : 0u;
                const uint64_t peers = digit_peers(d, valid, 8);
                if (valid && (peers & lanemask_lt()) == 0) atomicAdd(&cnt[d], (uint32_t)__popcll(peers));
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            // offsets + the next work list / leaves (adjacent small buckets
            // packed), collected in LDS; one reservation per list below (a
            // global atomic per entry from this one thread cost ~0.1 ms a segment)
            uint32_t acc = 0, leaf_lo = 0, leaf_n = 0, ne = 0;
            auto emit = [&](uint4 e, uint32_t kind) {
                s_ent[ne] = e;
                s_kind[ne] = (uint8_t)kind;
                ++ne;
            };
            auto flush = [&]() {
                if (leaf_n == 0) return;
                emit(make_uint4(lo + leaf_lo, leaf_n, seg.z, seg.w ^ 1u), leaf_n <= (uint32_t)CHUNK_CAP ? 0u : 1u);
                leaf_n = 0;
            };
            for (uint32_t d = 0; d < 256; ++d) {
                const uint32_t c = cnt[d];
                cur[d] = acc;
                if (c == 0) continue;
                if (c > (uint32_t)BIG_CAP) {
                    flush();
                    emit(make_uint4(lo + acc, c, seg.z, seg.w ^ 1u), last ? 3u : 2u);
                } else if (c > (uint32_t)CHUNK_CAP) {
                    flush();
                    leaf_lo = acc;
                    leaf_n = c;
                    flush();
                } else {
                    if (leaf_n + c > (uint32_t)CHUNK_CAP) flush();
                    if (leaf_n == 0) leaf_lo = acc;
                    leaf_n += c;
                }
                acc += c;
            }
            flush();
            uint32_t nk[4] = {0, 0, 0, 0};
            for (uint32_t e = 0; e < ne; ++e) s_rank[e] = nk[s_kind[e]]++;
            unsigned int* const ctrs[4] = {&ctr->n_leaf_small, &ctr->n_leaf_big, &ctr->n_seg[min(pass + 1, GIANT_PASSES)],
                                           &ctr->n_fallback};
            for (uint32_t k = 0; k < 4; ++k) s_base[k] = nk[k] ? atomicAdd(ctrs[k], nk[k]) : 0u;
            s_ne = ne;
        }
        __syncthreads();
        if (threadIdx.x < s_ne) {
            const uint32_t e = threadIdx.x, k = s_kind[e], at = s_base[k] + s_rank[e];
            uint4* const lists[4] = {gl.leaf_small, gl.leaf_big, gl.work[min(pass + 1, GIANT_PASSES)], gl.fallback};
            if (at < gl.cap) lists[k][at] = s_ent[e];
            else atomicOr(&ctr->err, ERR_SEGS);
        }
        // stable scatter, SPLIT_ITEMS x SPLIT_THREADS records a tile: wave w
        // ranks the contiguous records [w * 64 * SPLIT_ITEMS, +64 * SPLIT_ITEMS)
        // of the tile in order (its digit counts in wcnt[w], no block barrier
        // between items), one scan over the waves per digit, then the stores:
        // the leaves keep the arrival order -- first appearance -- so the
        // compact-key sort applies to them (two barriers per 4096 records; one
        // tile of 1024 with three cost pass 0 of the semi-tryptic split 2.4 ms)
        const uint32_t lane = lane_id();
        for (uint32_t t0 = 0; t0 < n; t0 += SPLIT_THREADS * SPLIT_ITEMS) {
            const uint32_t wb = t0 + w * 64 * SPLIT_ITEMS;
            Rec r[SPLIT_ITEMS];
            uint32_t dr[SPLIT_ITEMS];  // digit | rank in the wave's digit << 8
#pragma unroll
            for (uint32_t k = 0; k < SPLIT_ITEMS; ++k) {
                const uint32_t i = wb + k * 64 + lane;
                r[k] = i < n ? from[lo + i] : Rec{0, 0};
            }
#pragma unroll
            for (uint32_t k = 0; k < SPLIT_ITEMS; ++k) {
                const uint32_t i = wb + k * 64 + lane;
                const bool valid = i < n;
                const uint32_t d = valid ? (uint32_t)(key72(r[k]) >> sh) & 0xFFu : 0u;
                const uint64_t peers = digit_peers(d, valid, 8);
                const uint32_t before = wcnt[w][d];
                wave_sync();
                if (valid && (peers & lanemask_lt()) == 0) wcnt[w][d] = before + (uint32_t)__popcll(peers);
                wave_sync();
                dr[k] = valid ? d | ((before + (uint32_t)__popcll(peers & lanemask_lt())) << 8) : ~0u;
            }
            __syncthreads();
            if (threadIdx.x < 256) {  // per digit: the waves' bases in order, then the next tile's start
                uint32_t acc = cur[threadIdx.x];
                for (uint32_t q = 0; q < SPLIT_THREADS / 64; ++q) {
                    const uint32_t c = wcnt[q][threadIdx.x];
                    wcnt[q][threadIdx.x] = acc;
                    acc += c;
                }
                cur[threadIdx.x] = acc;
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < SPLIT_ITEMS; ++k)
                if (dr[k] != ~0u) to[lo + wcnt[w][dr[k] & 0xFFu] + (dr[k] >> 8)] = r[k];
            wave_sync();  // this wave's bases read: clear its row for the next tile
#pragma unroll
            for (uint32_t x = lane; x < 256; x += 64) wcnt[w][x] = 0;
            wave_sync();
        }
        __syncthreads();  // cur / cnt / wcnt reused by the next segment
    }
}

// leaves: sorted in LDS into out[lo, lo+n) (in place when they live in out);
// this launch takes the leaves of more than lmin records (the big leaves in
// two size classes, as the big tier: up to 3968 records two blocks per CU)
template <int NT, int CAP>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(CAP <= CHUNK_CAP ? DBI_MID_WPE : 4, 8)))
k_giant_leaf(const Rec* in, Rec* out, const uint4* __restrict__ list, const unsigned int* __restrict__ n_list,
             uint32_t cap, const uint8_t* __restrict__ res, const uint32_t* __restrict__ poff,
             uint32_t* __restrict__ ucount, Counters* __restrict__ ctr, uint32_t lmin) {
    __shared__ unsigned long long k0[CAP];
    __shared__ unsigned long long k1[CAP];
    __shared__ uint32_t aux[CAP];
    __shared__ uint32_t s_u32[NT / 64 + 1];
    __shared__ uint64_t s_min[NT / 64];
    __shared__ uint16_t s_tcnt[NT / 64 * 16];
    __shared__ uint32_t s_bad;
    const uint32_t nl = min(*n_list, cap);
    const RecLoc rl{res, poff, rec_width(ctr->max_plen)};
    for (uint32_t j = blockIdx.x; j < nl; j += gridDim.x) {
        const uint4 lf = list[j];
        if (lf.y <= lmin || lf.y > (uint32_t)CAP) continue;  // the other class's (block-uniform)
        const Rec* from = (lf.w ? out : in) + lf.x;
        const uint32_t h =
            bitonic_chunk<NT, CAP>(from, out + lf.x, lf.y, rl, k0, k1, aux, s_u32, &s_bad, s_min, s_tcnt);
        const uint32_t tot = block_sum<NT, uint32_t>(h, s_u32);
        if (threadIdx.x == 0) atomicAdd(&ucount[lf.z], tot);
        __syncthreads();
    }
}

// segments of one (mass, tag) key above BIG_CAP.  Up to FB_LDS records: the
// peptide repeated that often (semi-tryptic: one segment of ~9 000 records)
// is ordered by q1 alone -- q0 and the tag byte are the segment's -- in LDS
// (bitonic over the 8-B q1), its neighbours string-verified, and written with
// the one head; a segment holding more than one string (a 16-bit tag
// collision) or more records takes the global-memory path (process_chunk:
// (key, q1, index) bitonic in scratch, regroup by string).  The global path
// alone took 2.6 ms for the one 9 000-record segment (a single block, every
// bitonic step an L2 round trip).
constexpr uint32_t FB_LDS = 16384;
constexpr uint32_t FB_GROUPS = 64;  // string groups of one segment (hash table slots; at most half used)

// 64-bit hash of a peptide string (dword loads realigned to the string start,
// as seq_equal_at): equal strings hash equal whatever their alignment
__device__ __forceinline__ uint64_t seq_hash(const uint8_t* __restrict__ res, uint32_t g, uint32_t len) {
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(res) & 3u);
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(res - mis);
    const uint64_t ga = (uint64_t)g + mis;
    const uint64_t first = ga >> 2, last = (ga + len - 1) >> 2;
    const uint32_t sh = (uint32_t)(ga & 3u);
    uint64_t h = 0x9E3779B97F4A7C15ull ^ len;
    for (uint32_t k = 0; k < len; k += 4) {
        const uint64_t q = first + (k >> 2);
        const uint32_t x = __builtin_amdgcn_alignbyte(w[min(q + 1, last)], w[q], sh);
        const uint32_t rem = len - k;
        h = (h ^ (rem >= 4 ? x : x & ((1u << (8 * rem)) - 1u))) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 32;
    }
    return h;
}

// see k_giant_fallback; true when the segment was written (block-uniform)
__device__ bool fb_regroup(const Rec* __restrict__ in, Rec* __restrict__ out, uint32_t a, uint32_t m, uint64_t q0,
                           const RecLoc& rl, const unsigned long long* s_q, uint8_t* s_gid, unsigned long long* s_gh,
                           uint32_t* s_glead, uint32_t* s_gcnt, uint32_t* s_gbase, uint32_t* s_grun, uint32_t* s_gtile,
                           uint16_t (*s_wc)[FB_GROUPS], uint32_t* s_ng, uint32_t* s_bad, uint32_t* ucount) {
    constexpr uint32_t NT = BIG_THREADS, NW = NT / 64;
    constexpr unsigned long long EMPTY = ~0ull;
    const uint32_t tid = threadIdx.x, w = tid >> 6, lane = lane_id();
    for (uint32_t x = tid; x < FB_GROUPS; x += NT) {
        s_gh[x] = EMPTY;
        s_glead[x] = ~0u;
        s_gcnt[x] = 0;
        s_grun[x] = 0;
    }
    if (tid == 0) {
        *s_ng = 0;
        *s_bad = 0;
    }
    __syncthreads();
    for (uint32_t i = tid; i < m; i += NT) {
        const uint64_t q1 = s_q[i];
        const unsigned long long h = seq_hash(rl.res, rl.gstart(q1), q1_len(q1, rl.w)) & ~(1ull << 63);  // never EMPTY
        uint32_t sl = (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> 58), p = 0;
        for (; p < FB_GROUPS; ++p, sl = (sl + 1) & (FB_GROUPS - 1)) {
            const unsigned long long cur = s_gh[sl];
            if (cur == h) break;
            if (cur == EMPTY) {
                const unsigned long long prev = atomicCAS(&s_gh[sl], EMPTY, h);
                if (prev == EMPTY) {
                    atomicAdd(s_ng, 1u);
                    break;
                }
                if (prev == h) break;
            }
        }
        if (p == FB_GROUPS) {
            *s_bad = 1;
            sl = 0;
        }
        s_gid[i] = (uint8_t)sl;
        atomicMin(&s_glead[sl], i);
        atomicAdd(&s_gcnt[sl], 1u);
    }
    __syncthreads();
    if (*s_bad == 0 && *s_ng <= FB_GROUPS / 2)
        for (uint32_t i = tid; i < m; i += NT) {
            const uint32_t ld = s_glead[s_gid[i]];
            if (ld != i && !rl.same(Rec{q0, s_q[i]}, Rec{q0, s_q[ld]})) *s_bad = 1;  // a hash clash
        }
    __syncthreads();
    const bool ok = *s_bad == 0 && *s_ng <= FB_GROUPS / 2;
    if (!ok) {
        __syncthreads();  // every thread read s_bad / s_ng before the global path reuses nothing of this
        return false;
    }
    if (tid < FB_GROUPS) {  // groups in first-appearance order
        uint32_t base = 0;
        if (s_gcnt[tid])
            for (uint32_t t = 0; t < FB_GROUPS; ++t) base += (s_gcnt[t] && s_glead[t] < s_glead[tid]) ? s_gcnt[t] : 0u;
        s_gbase[tid] = base;
    }
    __syncthreads();
    // stable placement by group, one NT-record tile at a time (wave ranks in order)
    for (uint32_t t0 = 0; t0 < m; t0 += NT) {
        const uint32_t i = t0 + tid;
        const bool valid = i < m;
        const uint32_t g = valid ? s_gid[i] : 0u;
        s_wc[w][lane] = 0;
        wave_sync();
        const uint64_t peers = digit_peers(g, valid, 6);
        const uint32_t r = (uint32_t)__popcll(peers & lanemask_lt());
        if (valid && r == 0) s_wc[w][g] = (uint16_t)__popcll(peers);
        __syncthreads();
        if (tid < FB_GROUPS) {
            uint32_t acc = 0;
            for (uint32_t ww = 0; ww < NW; ++ww) {
                const uint32_t c = s_wc[ww][tid];
                s_wc[ww][tid] = (uint16_t)acc;
                acc += c;
            }
            s_gtile[tid] = acc;
        }
        __syncthreads();
        if (valid) {
            const uint32_t pos = s_gbase[g] + s_grun[g] + s_wc[w][g] + r;
            out[a + pos] = Rec{(q0 & ~0xFFull) | (pos == s_gbase[g] ? 1ull : 0ull), s_q[i]};
        }
        __syncthreads();
        if (tid < FB_GROUPS) s_grun[tid] += s_gtile[tid];
        __syncthreads();
    }
    if (tid == 0) atomicAdd(ucount, *s_ng);
    __syncthreads();
    (void)in;
    return true;
}

__global__ void __launch_bounds__(BIG_THREADS)
k_giant_fallback(Rec* in, Rec* out, const uint4* __restrict__ list, uint32_t cap, const uint8_t* __restrict__ res,
                 const uint32_t* __restrict__ poff, uint32_t* __restrict__ ucount, unsigned long long* ws_key,
                 uint32_t* ws_k2, Counters* __restrict__ ctr) {
    __shared__ uint32_t s_u32[BIG_THREADS / 64 + 1];
    __shared__ unsigned long long s_flag;
    __shared__ unsigned long long s_q[FB_LDS];
    // string regroup of a collision segment: group of each record, hash table,
    // per-group leader (first position) / count / base / running count, per-(wave, group) tile counts
    __shared__ uint8_t s_gid[FB_LDS];
    __shared__ unsigned long long s_gh[FB_GROUPS];
    __shared__ uint32_t s_glead[FB_GROUPS], s_gcnt[FB_GROUPS], s_gbase[FB_GROUPS], s_grun[FB_GROUPS], s_gtile[FB_GROUPS];
    __shared__ uint16_t s_wc[BIG_THREADS / 64][FB_GROUPS];
    __shared__ uint32_t s_ng, s_bad;
    const uint32_t nl = min(ctr->n_fallback, cap);
    const RecLoc rl{res, poff, rec_width(ctr->max_plen)};
    for (uint32_t j = blockIdx.x; j < nl; j += gridDim.x) {
        const uint4 sg = list[j];
        const uint32_t a = sg.x, m = sg.y;
        if (sg.w) {  // lives in out: move it back to in (free there) so out is written once
            for (uint32_t i = threadIdx.x; i < m; i += BIG_THREADS) in[a + i] = out[a + i];
            __syncthreads();
        }
        if (m <= FB_LDS) {
            const Rec r0 = in[a];
            uint32_t P2 = 1;
            while (P2 < m) P2 <<= 1;
            bool diff = false;
            for (uint32_t i = threadIdx.x; i < P2; i += BIG_THREADS) {
                unsigned long long q = ~0ull;  // padding sorts last
                if (i < m) {
                    const Rec r = in[a + i];
                    diff |= r.q0 != r0.q0 || (r.q1 >> 56) != (r0.q1 >> 56);
                    q = r.q1;
                }
                s_q[i] = q;
            }
            if (threadIdx.x == 0) s_flag = 0;
            if (!__syncthreads_or(diff)) {  // one (mass, tag) key (block-uniform)
                for (uint32_t k = 2; k <= P2; k <<= 1) {
                    for (uint32_t h = k >> 1; h > 0; h >>= 1) {
                        for (uint32_t i = threadIdx.x; i < P2; i += BIG_THREADS) {
                            const uint32_t ix = i ^ h;
                            if (ix > i) {
                                const unsigned long long x = s_q[i], y = s_q[ix];
                                if (((i & k) == 0) ? x > y : x < y) {
                                    s_q[i] = y;
                                    s_q[ix] = x;
                                }
                            }
                        }
                        __syncthreads();
                    }
                }
                for (uint32_t i = threadIdx.x + 1; i < m; i += BIG_THREADS)
                    if (!rl.same(Rec{r0.q0, s_q[i]}, Rec{r0.q0, s_q[i - 1]})) s_flag = 1;
                __syncthreads();
                const bool one_string = s_flag == 0;
                if (one_string) {
                    for (uint32_t i = threadIdx.x; i < m; i += BIG_THREADS)
                        out[a + i] = Rec{(r0.q0 & ~0xFFull) | (i == 0 ? 1ull : 0ull), s_q[i]};
                    if (threadIdx.x == 0) atomicAdd(&ucount[sg.z], 1u);
                }
                __syncthreads();  // every thread read s_flag / s_q before the next use
                if (one_string) continue;
                // several strings (a tag collision): group by a string hash in
                // LDS, verify every record against its group's first one,
                // groups in first-appearance order, q1 order inside a group
                // (what process_chunk's regroup computes with an O(n^2) leader
                // search); more than FB_GROUPS / 2 strings or a hash clash
                // between different strings: the global path
                if (fb_regroup(in, out, a, m, r0.q0, rl, s_q, s_gid, s_gh, s_glead, s_gcnt, s_gbase, s_grun,
                               s_gtile, s_wc, &s_ng, &s_bad, ucount + sg.z))
                    continue;
            }
        }
        unsigned long long* key = ws_key + 4ull * a;
        unsigned long long* hsh = key + 2ull * m;
        uint32_t* k2 = ws_k2 + 4ull * a;
        uint32_t* k3 = k2 + 2ull * m;
        const uint32_t h = process_chunk<BIG_THREADS>(in + a, out + a, m, rl, key, hsh, k2, k3, s_u32, &s_flag);
        const uint32_t tot = block_sum<BIG_THREADS, uint32_t>(h, s_u32);
        if (threadIdx.x == 0) atomicAdd(&ucount[sg.z], tot);
        __syncthreads();
    }
}

hipError_t launch_giant_chunks(const Rec* d_in, Rec* d_out, const uint32_t* d_chunk_lo, const uint8_t* d_res,
                               const uint32_t* d_poff, uint32_t* d_ucount, const uint32_t* d_giant_list,
                               uint4* d_segs, size_t seg_cap, unsigned long long* d_ws_key, uint32_t* d_ws_k2,
                               Counters* d_ctr, hipStream_t s) {
    GiantLists gl;
    for (int p = 0; p <= GIANT_PASSES; ++p) gl.work[p] = d_segs + (size_t)p * seg_cap;
    gl.leaf_small = d_segs + (size_t)(GIANT_PASSES + 1) * seg_cap;
    gl.leaf_big = gl.leaf_small + seg_cap;
    gl.fallback = gl.leaf_big + seg_cap;
    gl.cap = (uint32_t)std::min<size_t>(seg_cap, 0xFFFFFFFFu);
    Rec* in = const_cast<Rec*>(d_in);  // the radix output: free scratch once the chunk sort read it
    // (work lists are counted in ctr->n_seg, zeroed with the counters at the start of the build)
    DBI_LAUNCH(k_giant_init, dim3(64), dim3(256), 0, s, d_giant_list, d_chunk_lo, d_ucount, gl, d_ctr);
    for (int p = 0; p < GIANT_PASSES; ++p)
        DBI_LAUNCH(k_giant_split, dim3(512), dim3(SPLIT_THREADS), 0, s, in, d_out, gl, p, d_ctr);
    DBI_LAUNCH((k_giant_leaf<CHUNK_THREADS, CHUNK_CAP>), dim3(2048), dim3(CHUNK_THREADS), 0, s, in, d_out,
               gl.leaf_small, &d_ctr->n_leaf_small, gl.cap, d_res, d_poff, d_ucount, d_ctr, 0u);
    DBI_LAUNCH((k_giant_leaf<BIG_THREADS / 2, BIG_CAP / 2>), dim3(512), dim3(BIG_THREADS / 2), 0, s, in, d_out,
               gl.leaf_big, &d_ctr->n_leaf_big, gl.cap, d_res, d_poff, d_ucount, d_ctr, 0u);
    DBI_LAUNCH((k_giant_leaf<BIG_THREADS, BIG_CAP>), dim3(256), dim3(BIG_THREADS), 0, s, in, d_out, gl.leaf_big,
               &d_ctr->n_leaf_big, gl.cap, d_res, d_poff, d_ucount, d_ctr, (uint32_t)(BIG_CAP / 2));
    DBI_LAUNCH(k_giant_fallback, dim3(256), dim3(BIG_THREADS), 0, s, in, d_out, gl.fallback, gl.cap, d_res, d_poff,
               d_ucount, d_ws_key, d_ws_k2, d_ctr);
    return hipGetLastError();
}

}  // namespace dbi
