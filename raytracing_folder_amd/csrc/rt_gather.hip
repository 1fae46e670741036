// rt_gather.hip -- K5, the k-nearest photon gather (k_gather) and its launch (rtk_launch_gather): gfx950 / CDNA4, wave64.
// Compiled with -ffp-contract=off like the other kernels; only the photon loop opts into contraction (RT_FP_CONTRACT).
#include <hip/hip_runtime.h>
#include <math.h>
#include "rt_launch.h"
#include "rt_kernel_util.h"

// k_gather tuning knobs (the defaults are the measured best on MI355X)
#ifndef RT_GATHER_GUESS
#define RT_GATHER_GUESS 1.2f   // photons expected inside the first trial radius, in units of k (round 2, sub-leaves: 1.1: 42.0 ms, 1.15: 40.8, 1.2: 40.7, 1.3: 41.7, 1.45: 43.3)
#endif
#ifndef RT_GATHER_RING
#define RT_GATHER_RING 128     // LDS entries for the photons around the predicted k-th distance (0: always re-read in pass 2)
#endif
#ifndef RT_GATHER_BAND_LO
#define RT_GATHER_BAND_LO 0.92f   // the ring keeps the photons between BAND_LO and BAND_HI times the predicted k-th squared distance
                                  // (0.85-1.18: 40.7 ms, 0.88-1.15: 39.7, 0.92-1.10: 39.4, 0.94-1.08: 39.3)
#endif
#ifndef RT_GATHER_BAND_HI
#define RT_GATHER_BAND_HI 1.10f
#endif
#ifndef RT_GATHER_BATCH
#define RT_GATHER_BATCH 32     // queries a wave lists per phase A (40 leaf ids each: lists + ring keep 5 waves/SIMD)
#endif
#ifndef RT_GATHER_CELL_GUESS
#define RT_GATHER_CELL_GUESS RT_GATHER_GUESS    // first trial radius^2 of a query whose cell remembers a k-th distance: that distance times this
#endif
// the photon loop of k_gather may contract mul+add into fma (d^2, dir.N, box distances, weighted sums; gate there: 2e-5); the rest of the
// gather (first radius, area, normalisation, the weighted add into the sample) stays uncontracted like every other kernel
#define RT_FP_CONTRACT _Pragma("clang fp contract(fast)")
#define RT_SUBS_PER_STEP (64 / RT_SUB_PHOTONS)                  // sub-leaves a wavefront examines per step
#define RT_SUBLIST_CAP (RT_LEAFLIST_CAP * RT_LEAF_SUBS)         // sub-leaf ids of one query

// ------------------------------------------------------------------------------------------------
// K5: PhotonMap::EstimateIrradiance<k>(irr, dir, radius, pos, &N, 1, CONSTANT)
// (FIN/include/cyPhotonMap.h:288-336, LocatePhotons :365-440).
//
// The reference walks its heap-ordered kd-tree recursively per query and keeps the k nearest
// accepted photons (inside the radius, photonDir.N < 0) in a max-heap, shrinking the search radius
// once the heap is full; the estimate only needs
//   sum of power, sum of dir*maxPower over that set, and r_k^2 (= radius^2 while at most k photons
//   qualify, else the k-th smallest squared distance).
// Here a wavefront claims a batch of RT_GATHER_BATCH (32) queries at a time (claim_batch), one per lane of its lower
// half, and picks each one's first trial radius from the density grid (first_radius).  Then, until all are answered:
//   Phase A, one query per lane pair (list_leaves): a stackless walk of the complete binary tree of leaf boxes lists
//     the leaves within the query's CURRENT trial radius (ids in LDS).
//   Phase B, the whole wave per pending query:
//     compact   the sub-leaves of the listed leaves that the ball cuts, ids in LDS (compact_subleaves).  A pass over them
//               reads 64 / RT_SUB_PHOTONS (4) sub-leaves of RT_SUB_PHOTONS (16) photon slots per step, lane = slot.
//     pass 1    counts the accepted photons into a 256-bin histogram of a 24-bit fixed-point distance key (LDS atomics),
//               sums those safely below the predicted k-th distance and parks the ones around it in an LDS ring.
//     decide    if the trial radius is smaller than the requested one and at most k photons qualified, the query is
//               retried in the next round with a larger radius predicted from the count (photons lie on surfaces:
//               count ~ r^2); a trial that finds MORE than k is exact, because the k nearest all lie inside it.
//     select    if more than k qualify, the bin holding the k-th is located with a wave scan (locate_kth: one more
//               8-bit level while the bin holds more than 64); the bins below it are summed and that bin is collected
//               for an exact rank selection -- from the ring, or by pass 2 over the sub-leaves when the ring cannot serve.
//     finish    the six sums and r_k^2 go to the query's lane (deliver); area, normalisation and output for all the
//               queries a round answered at once (finish_queries).
// Sums are per-lane partials combined by a fixed butterfly: deterministic.
// ------------------------------------------------------------------------------------------------
struct GatherArgs {
    DevPhotonMap pm;
    const float4 *qa, *qb, *qc;      // query queue
    const uint32_t *count_ptr;       // number of queries (device)
    uint32_t *next_batch;            // zero at launch, RT_CTR_STRIDE apart: [seg] = batches handed out of XCD segment seg (8), [8] = mask of the segments used up
    uint32_t count_cap;
    int k; float radius;
    float *sample_rgb;               // mode 0: atomicAdd w * irr * max(0, N.(-dir)) into the slot
    float *out_irr, *out_dir;        // mode 1: write irr[3], dir[3] per query (rt_estimate_irradiance)
    int mode;
    unsigned long long *stats;
    float *cell_rk2;                 // per density-grid cell: the k-th squared distance of the last query answered there (0 = none yet); may be NULL
    unsigned long long *fx;          // reproducible instantiation, mode 0: deposit into this secondary plane (fx_add) instead of sample_rgb
};

// Wave-wide inclusive scans on the DPP path (row_shr 1/2/4/8 inside each row of 16 lanes, then
// row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3): six VALU instructions, no LDS
// crossbar traffic (__shfl is ds_bpermute: an LDS round trip per step).  All 64 lanes must be active.
// Lanes without a source keep `old` = the identity.  Fixed order => deterministic float sums.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f(float identity, float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(x), CTRL, ROW_MASK, 0xF, false));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_u(uint32_t identity, uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)x, CTRL, ROW_MASK, 0xF, false);
}
#define DPP_ROW_SHR(n) (0x110 + (n))
#define DPP_ROW_BCAST15 0x142
#define DPP_ROW_BCAST31 0x143
__device__ __forceinline__ uint32_t wave_scan_add_u(uint32_t x)
{
    x += dpp_u<DPP_ROW_SHR(1), 0xF>(0u, x); x += dpp_u<DPP_ROW_SHR(2), 0xF>(0u, x);
    x += dpp_u<DPP_ROW_SHR(4), 0xF>(0u, x); x += dpp_u<DPP_ROW_SHR(8), 0xF>(0u, x);
    x += dpp_u<DPP_ROW_BCAST15, 0xA>(0u, x); x += dpp_u<DPP_ROW_BCAST31, 0xC>(0u, x);
    return x;
}
__device__ __forceinline__ float wave_scan_max0(float x)          // x >= 0
{
    x = fmaxf(x, dpp_f<DPP_ROW_SHR(1), 0xF>(0.0f, x)); x = fmaxf(x, dpp_f<DPP_ROW_SHR(2), 0xF>(0.0f, x));
    x = fmaxf(x, dpp_f<DPP_ROW_SHR(4), 0xF>(0.0f, x)); x = fmaxf(x, dpp_f<DPP_ROW_SHR(8), 0xF>(0.0f, x));
    x = fmaxf(x, dpp_f<DPP_ROW_BCAST15, 0xA>(0.0f, x)); x = fmaxf(x, dpp_f<DPP_ROW_BCAST31, 0xC>(0.0f, x));
    return x;
}
// total: lane 63 of the inclusive scan, as a scalar
__device__ __forceinline__ float wave_max0(float x) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_scan_max0(x)), 63)); }

// Six wave totals at once.  v_permlane32_swap / v_permlane16_swap (gfx950) exchange half-waves / odd-even rows of TWO
// registers, so one swap + one add folds two values at a time: after the 32-lane and the 16-lane fold four values share
// one register (a row of 16 lanes each), and the last four steps (row_shr 8, 4, 2, 1) run on two registers instead of
// six: 25 vector instructions instead of 48 for six separate scans.  Fixed order => deterministic.
__device__ __forceinline__ void fold32(float a, float b, float &ab)
{
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    ab = __uint_as_float(r[0]) + __uint_as_float(r[1]);          // lanes 0-31: a folded, lanes 32-63: b folded
}
__device__ __forceinline__ void fold16(float x, float y, float &xy)
{
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    xy = __uint_as_float(r[0]) + __uint_as_float(r[1]);          // rows 0..3: x.lo, y.lo, x.hi, y.hi folded to 16 lanes
}
__device__ __forceinline__ float row_total(float x)               // lane 15 of every row: the row's sum
{
    x += dpp_f<DPP_ROW_SHR(8), 0xF>(0.0f, x); x += dpp_f<DPP_ROW_SHR(4), 0xF>(0.0f, x);
    x += dpp_f<DPP_ROW_SHR(2), 0xF>(0.0f, x); x += dpp_f<DPP_ROW_SHR(1), 0xF>(0.0f, x);
    return x;
}
__device__ __forceinline__ void wave_sum6(float v0, float v1, float v2, float v3, float v4, float v5, float out[6])
{
    float s01, s23, s45, t0123, t45;
    fold32(v0, v1, s01); fold32(v2, v3, s23); fold32(v4, v5, s45);
    fold16(s01, s23, t0123);          // rows: v0, v2, v1, v3
    fold16(s45, s45, t45);            // rows: v4, v4, v5, v5
    t0123 = row_total(t0123); t45 = row_total(t45);
    out[0] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t0123), 15));
    out[2] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t0123), 31));
    out[1] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t0123), 47));
    out[3] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t0123), 63));
    out[4] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t45), 15));
    out[5] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t45), 47));
}

// value of lane l (wave-uniform l) as a scalar: v_readlane, no LDS traffic, result lives in an SGPR
__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ uint32_t lane_u(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

// boxes are two aligned 16-byte words (lo.xyz, -), (hi.xyz, -): one visit = two dwordx4 loads
__device__ __forceinline__ float box_dist2(const float4 *b, float px, float py, float pz)
{
    RT_FP_CONTRACT
    const float4 lo = b[0], hi = b[1];
    const float dx = fmaxf(fmaxf(lo.x - px, px - hi.x), 0.0f);
    const float dy = fmaxf(fmaxf(lo.y - py, py - hi.y), 0.0f);
    const float dz = fmaxf(fmaxf(lo.z - pz, pz - hi.z), 0.0f);
    return dx * dx + dy * dy + dz * dz;
}

// LDS hand-off between lanes of ONE wavefront: LDS operations of a wave complete in issue order, so
// only the compiler has to be kept from reordering, plus a wait for outstanding LDS returns.
__device__ __forceinline__ void wave_sync()
{
    // "wavefront" scope: the hardware already executes one wave's LDS instructions in issue order, so a write by one lane is
    // seen by a later read of another lane of the SAME wave without waiting for anything; the fences only keep the compiler
    // from moving LDS accesses across this point.  ("workgroup" scope made every one of the ~10 hand-offs per query an
    // s_waitcnt vmcnt(0) lgkmcnt(0): it also drained the photon loads in flight.)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct GatherLds {
    uint16_t leaves[RT_GATHER_BATCH][RT_LEAFLIST_CAP];   // per query (lane) leaf ids
    uint32_t subs[RT_SUBLIST_CAP + RT_SUBS_PER_STEP];    // the current query's sub-leaf ids, padded to whole steps with the dummy sub-leaf
    union alignas(16) {                                  // never live at the same time:
        uint32_t hist[256];                              //   the distance-key histogram while the k-th photon's bin is located
        struct { float sel_d[64]; uint32_t sel_i[64]; uint32_t sel_n; };   //   then that bin's photons for the exact rank selection
    };
    // everything pass 1 read about a photon whose distance lies in the band around the predicted k-th one,
    // so that the exact selection does not have to read the leaves a second time
    float4   ring_a[RT_GATHER_RING];      // d2, dir.x, dir.y, dir.z
    float2   ring_b[RT_GATHER_RING];      // max power, colour bytes
};

// Color24 -> Color (cyColor.h): byte / 255.0f, correctly rounded, without the ~10-instruction IEEE division and without
// a table: 1/255 as a two-term constant, r_hi = RN(1/255) and r_lo = RN(1/255 - r_hi); fma(c, r_hi, RN(c * r_lo)) adds the
// exact product c * r_hi to a correction that is itself good to 2^-48 of the result, and lands on the correctly rounded
// quotient for every byte value (all 256 checked exactly, in rational arithmetic: tests/test_host.py; on the device:
// test_gpu_parity.py::test_irradiance_single_photon_colour_bytes).  Two instructions; c * RN(1/255) alone is wrong for
// 121 of the 256 bytes, and the Newton form used before took three.
__device__ __forceinline__ float byte_over_255(uint32_t c)
{
    const float r_hi = 0x1.010102p-8f, r_lo = -0x1.fdfdfep-33f;
    const float x = (float)c;
    return __fmaf_rn(x, r_hi, x * r_lo);
}

// one lane's photon of one sub-leaf against one query (the test of LocatePhotons :383-392).  d2 is the squared distance
// for a photon that faces the surface and +infinity for one that does not (or for an empty slot, whose position is
// 3e38): "accepted" is then the single compare d2 < rq2, and every narrower test (below t_lo, inside the band) is one
// compare as well -- a compare's lane mask is its ballot, while a ballot of a combined condition costs two more
// vector instructions, on the unit this kernel is bound by.
struct Cand { float d2; float4 pa, pb; };
struct GatherQuery { float px, py, pz, nx, ny, nz, rq2, kscale; };
__device__ __forceinline__ Cand make_cand(float4 pa, float4 pb, const GatherQuery &Q)
{
    RT_FP_CONTRACT
    Cand c;
    c.pa = pa; c.pb = pb;
    const float dfx = pa.x - Q.px, dfy = pa.y - Q.py, dfz = pa.z - Q.pz;       // dif = p.position - np.pos
    const float d2 = dfx * dfx + dfy * dfy + dfz * dfz;                         // LengthSquared
    const bool away = (pa.w * Q.nx + pb.x * Q.ny + pb.y * Q.nz) >= 0;           // dir.N >= 0 rejects
    c.d2 = away ? __builtin_inff() : d2;                                        // dist2 < dist2[0] is tested by the caller
    return c;
}
// 24-bit fixed-point distance key of an ACCEPTED photon: kscale = 16777000 / rq2, so d2 < rq2 gives at most
// 16777000 * (1 + 2^-22) < 2^24 whatever the roundings
__device__ __forceinline__ uint32_t cand_key(const Cand &c, const GatherQuery &Q) { return (uint32_t)(c.d2 * Q.kscale); }

// Visit every photon slot of the n_sub sub-leaves listed in LDS (ids[]; padded to whole steps with the dummy sub-leaf,
// whose slots are all empty), 64 / RT_SUB_PHOTONS (4) sub-leaves per step (lanes 0-15 the first, 16-31 the second, ...):
// f(candidate, slot) is called wave-uniformly (all 64 lanes) so it may use ballots.  A lane's share of a step is one LDS
// read (its sub-leaf id), one shift-or (the byte offset, 32 bits) and two coalesced 16-byte loads from scalar bases --
// nothing else is fetched per photon.  The loads of step it+1 are issued before step it is processed, so a wave
// always has a step in flight while it works: measured on MI355X the un-pipelined version spent 78 % of its wave
// cycles parked on s_waitcnt (SQ_WAIT_ANY / SQ_WAVE_CYCLES).
template <class F>
__device__ __forceinline__ void scan_subleaves(const DevPhotonMap &pm, const uint32_t *ids, uint32_t n_sub, int lane,
                                               const GatherQuery &Q, F &&f)
{
    if (n_sub == 0) return;
    const uint32_t n_iter = (n_sub + RT_SUBS_PER_STEP - 1u) / RT_SUBS_PER_STEP;
    const uint32_t *mine = ids + (uint32_t)lane / RT_SUB_PHOTONS;           // which of a step's sub-leaves this lane reads
    const uint32_t lane_off = ((uint32_t)lane % RT_SUB_PHOTONS) * 16u;
    const char *pa = (const char *)pm.pa, *pb = (const char *)pm.pb;
    auto ld = [&](uint32_t it, float4 &a, float4 &b, uint32_t &slot) {
        const uint32_t off = (mine[RT_SUBS_PER_STEP * it] * (RT_SUB_PHOTONS * 16u)) | lane_off;   // < 2^32: checked at upload
        slot = off;
        a = *(const float4 *)(pa + off);
        b = *(const float4 *)(pb + off);
    };
    // two register sets used alternately, each refilled right after it was consumed; the reload index
    // is clamped instead of branched over (the last step may be fetched twice) so that neither set
    // is a loop-carried copy of the other
    float4 a0, b0, a1, b1;
    uint32_t s0, s1;
    ld(0u, a0, b0, s0);
    uint32_t it = 0;
    for (; it + 1 < n_iter; it += 2) {
        ld(it + 1, a1, b1, s1);
        f(make_cand(a0, b0, Q), s0);
        ld(min(it + 2, n_iter - 1), a0, b0, s0);
        f(make_cand(a1, b1, Q), s1);
    }
    if (it < n_iter) f(make_cand(a0, b0, Q), s0);
}

// ------------------------------------------------------------------------------------------------
// state
// ------------------------------------------------------------------------------------------------
// The query a lane holds (lanes 0 .. RT_GATHER_BATCH-1 of a batch), from the queue until its result is written.
struct LaneQuery {
    float4 a, b, c;                  // the queue record: a = (pos.xyz, N.x), b = (N.yz, weight.rg), c = (weight.b, sample slot, -, -)
    uint32_t qi;                     // its index in the queue
    bool pending, finish;            // not answered yet; answered in this round: the f_* below wait for finish_queries
    float r2cur;                     // the trial radius^2 of its next round
    float cell_pred;                 // what its grid cell remembers: > 0 the k-th squared distance of the cell's last query, < 0 "sparse here", 0 nothing
    uint32_t cell_index, walk_start; // that cell; where the query's tree walk starts (DevPhotonMap::cell_start)
    float f_pr, f_pg, f_pb, f_dx, f_dy, f_dz, f_area;     // the six sums and dist2[0] (negative: no photon at all)
};

// One query as the whole wave sees it during phase B (everything wave-uniform but `lane`): the point, and its sub-leaves.
struct QueryPass {
    const DevPhotonMap &pm; GatherLds &L; int lane;
    GatherQuery Q;
    bool slow;                       // the leaf list overflowed its LDS row: no sub-leaf list either, every pass tests ALL sub-leaf boxes
    uint32_t n_sub;                  // sub-leaves the query ball cuts
};

// Per-lane partial sums over the photons that count: power (GetPower = Color24 -> Color times max power) and dir * maxPower.
// A photon is added under a branch of the caller; the branch-free form (adding exact zeros for the others) measured slower.
struct GatherSums {
    float pr, pg, pb, dx, dy, dz;
    __device__ __forceinline__ void clear() { pr = pg = pb = dx = dy = dz = 0; }
    __device__ __forceinline__ void add(float dirx, float diry, float dirz, float maxp, uint32_t cbits)
    {
        RT_FP_CONTRACT
        pr += byte_over_255(cbits & 255u) * maxp; pg += byte_over_255((cbits >> 8) & 255u) * maxp; pb += byte_over_255((cbits >> 16) & 255u) * maxp;
        dx += dirx * maxp; dy += diry * maxp; dz += dirz * maxp;
    }
    __device__ __forceinline__ void add(const float4 &pa, const float4 &pb_) { add(pa.w, pb_.x, pb_.y, pb_.z, __float_as_uint(pb_.w)); }
};

// wave-uniform tallies of a wave's whole run (rt_stats)
struct GatherTally {
    unsigned long long visited;      // sub-leaves examined by first passes
    uint32_t n_rounds, n_slow;       // query rounds, and those on the slow path
    uint32_t n_reads;                // sub-leaves read, re-reads included
};

// the band around the predicted k-th squared distance: pass 1 sums what lies below t_lo at once and parks [t_lo, t_hi) in the ring
struct GatherBand { float t_lo, t_hi; };

// where the k-th nearest photon's key lies: in the bin `prefix` of the level whose digit is (key >> shift) & 255
struct KthBin {
    uint32_t need, in_bin;           // rank (1-based) of the k-th inside the bin; photons in the bin
    uint32_t prefix; int shift;      // key bits fixed so far
    __device__ __forceinline__ uint32_t mask() const { return ~((1u << shift) - 1u) & 0xFFFFFFu; }
};

#define RT_GATHER_NO_BATCH 0xFFFFFFFFu

// ------------------------------------------------------------------------------------------------
// claiming work
// ------------------------------------------------------------------------------------------------
// XCD affinity: the queue is in sample order, so neighbouring batches look up neighbouring points and read the
// same sub-leaves.  The queue is cut into eight contiguous segments, one per XCD: the waves of an XCD (640 of
// them) then work inside a narrow window of the queue at any time and share its photons through their XCD's
// 4 MB L2 instead of each XCD streaming every window's photons from the Infinity Cache.  A wave whose segment
// is used up takes batches from the next ones (query cost varies 100x: no static split).  Speed only: any
// assignment gives the same results.
__device__ __forceinline__ uint32_t home_segment()
{
    uint32_t xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    return xcc & 7u;
}

// The first query of the next batch of RT_GATHER_BATCH queries for this wave, or RT_GATHER_NO_BATCH when all segments are used up.
// Batches are handed out dynamically (one atomic per batch): query cost varies by two orders of magnitude with the local
// photon density, so a static split leaves a long tail.  `seg` is the segment the wave is taking from; it moves on here.
// A wave that finds a segment used up says so in a mask the others READ before they try it: without it every wave ends with
// eight failing atomics -- 41 000 of them queueing at the memory side (device-scope atomics are executed there, one after the
// other per channel) while nothing else is left to do.  The counters sit RT_CTR_STRIDE apart for the same reason (rt_dev.h).
// Measured and not kept (r4, profiles/r04_experiments.json): the last batches of a segment handed out as 8-query units, a
// segment handed out from its end.
__device__ __forceinline__ uint32_t claim_batch(const GatherArgs &G, int lane, uint32_t n_batches, uint32_t &seg)
{
    const uint32_t seg_len = (n_batches + 7u) / 8u;
    for (;;) {
        const uint32_t seg_first = seg * seg_len;
        const uint32_t seg_size = seg_first >= n_batches ? 0u : min(seg_len, n_batches - seg_first);
        uint32_t got = 0;
        if (lane == 0) got = atomicAdd(G.next_batch + seg * RT_CTR_STRIDE, 1u);
        got = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
        if (got < seg_size) return (seg_first + got) * (uint32_t)RT_GATHER_BATCH;
        // this segment is finished: move on to one that is not known to be, or stop
        uint32_t *const done_mask = G.next_batch + 8 * RT_CTR_STRIDE;
        uint32_t done = 0;                               // (what this wave marked earlier is in the mask it reads: same address, program order)
        if (lane == 0) {
            done = __hip_atomic_load(done_mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!((done >> seg) & 1u)) atomicOr(done_mask, 1u << seg);
        }
        done = ((uint32_t)__builtin_amdgcn_readfirstlane((int)done) | (1u << seg)) & 255u;
        if (done == 255u) return RT_GATHER_NO_BATCH;
        const uint32_t rot = ((done ^ 255u) | ((done ^ 255u) << 8)) >> (seg + 1u);     // segments still open, seen from seg + 1
        seg = (seg + 1u + ((uint32_t)__ffs((int)rot) - 1u)) & 7u;
    }
}

// lane l < RT_GATHER_BATCH takes query qbase + l of the queue (if there is one)
__device__ __forceinline__ LaneQuery load_query(const GatherArgs &G, int lane, uint32_t qbase, uint32_t nq)
{
    LaneQuery q;
    q.qi = qbase + lane;
    q.pending = lane < RT_GATHER_BATCH && q.qi < nq;
    q.a = make_float4(0, 0, 0, 0); q.b = make_float4(0, 0, 0, 0); q.c = make_float4(0, 0, 0, 0);
    if (q.pending) { q.a = G.qa[q.qi]; q.b = G.qb[q.qi]; q.c = G.qc[q.qi]; }
    q.f_pr = q.f_pg = q.f_pb = q.f_dx = q.f_dy = q.f_dz = 0; q.f_area = -1.0f; q.finish = false;
    return q;
}

// First trial radius from the density grid: about RT_GATHER_GUESS * k photons expected inside (count ~ r^2 on a surface through a
// cell of side h: c photons per h^2; guess_c = RT_GATHER_GUESS * k * h^2 / pi).  Also what the query's cell remembers, and where
// its tree walk starts.
__device__ __forceinline__ void first_radius(const GatherArgs &G, LaneQuery &q, float r2, float guess_c)
{
    q.r2cur = r2; q.cell_pred = 0.0f; q.cell_index = 0; q.walk_start = 1;
    if (!(q.pending && G.pm.n_leaves > 1)) return;
    const float fx = (q.a.x - G.pm.grid_min[0]) * G.pm.inv_cell, fy = (q.a.y - G.pm.grid_min[1]) * G.pm.inv_cell, fz = (q.a.z - G.pm.grid_min[2]) * G.pm.inv_cell;
    const int gx = min(max((int)fx, 0), G.pm.grid_dim[0] - 1);
    const int gy = min(max((int)fy, 0), G.pm.grid_dim[1] - 1);
    const int gz = min(max((int)fz, 0), G.pm.grid_dim[2] - 1);
    q.cell_index = (uint32_t)(((size_t)gz * G.pm.grid_dim[1] + gy) * G.pm.grid_dim[0] + gx);
    // only for a point that really lies in its cell (points outside the photons' bounding box are clamped to the rim)
    const bool in_grid = fx >= 0.0f && fy >= 0.0f && fz >= 0.0f && (int)fx == gx && (int)fy == gy && (int)fz == gz;
    if (G.pm.cell_start && in_grid && G.radius <= G.pm.start_radius) q.walk_start = G.pm.cell_start[q.cell_index];
    const uint32_t cnt = G.pm.grid[q.cell_index];
    q.r2cur = fminf(fmaxf(guess_c / (float)(cnt > 0u ? cnt : 1u), r2 * 1.0e-4f), r2);
    if (G.cell_rk2) {
        q.cell_pred = G.cell_rk2[q.cell_index];
        // a cell that has seen a query also knows a better first radius than the density estimate: a little above its k-th distance
        if (q.cell_pred > 0.0f) q.r2cur = fminf(fmaxf(q.cell_pred * RT_GATHER_CELL_GUESS, r2 * 1.0e-4f), r2);
        else if (q.cell_pred < 0.0f) q.r2cur = r2;       // "sparse here": the full radius at once
    }
}

// ------------------------------------------------------------------------------------------------
// phase A: pending lanes list the leaves inside their trial radius
// ------------------------------------------------------------------------------------------------
// Two lanes walk for one query: lane l and lane l + 32 hold the same point and radius, keep the same walk state
// and split the box tests of every visit between them (grandchildren 0-1 / 2-3, child 0 / 1); one
// v_permlane32_swap per visit gives both the combined result.  The queries sit in lanes 0-31 only (32 per
// batch), so the upper half of the wave would otherwise idle through the phase.
// Returns the number of leaves the lane's query ball cuts; the first RT_LEAFLIST_CAP ids are in L.leaves[lane].
__device__ __forceinline__ uint32_t list_leaves(const DevPhotonMap &pm, GatherLds &L, int lane, const LaneQuery &q)
{
    static_assert(RT_GATHER_BATCH == 32, "phase A pairs lane l with lane l + 32");
    const uint32_t n_leaves = pm.n_leaves;
    const bool upper = lane >= 32;
    auto from_lower = [](float v) { return __uint_as_float(__builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false)[0]); };
    const float wx = from_lower(q.a.x), wy = from_lower(q.a.y), wz = from_lower(q.a.z), wr2 = from_lower(q.r2cur);
    const uint32_t wstart = __builtin_amdgcn_permlane32_swap(q.walk_start, q.walk_start, false, false)[0];
    const bool walking = ((uint32_t)ballot64(q.pending) >> (lane & 31)) & 1u;
    auto both_halves = [](uint32_t mine, int bits) {       // my half's result bits -> lower half's | upper half's << bits, in every lane
        const auto r = __builtin_amdgcn_permlane32_swap(mine, mine, false, false);
        return r[0] | (r[1] << bits);
    };
    uint32_t nl = 0;
    auto list_leaf = [&](uint32_t leaf) {
        if (!upper && nl < RT_LEAFLIST_CAP) L.leaves[lane][nl] = (uint16_t)leaf;
        nl++;
    };
    if (!(walking && n_leaves)) return nl;
    // Depth-first, left to right (ascending leaf ids).  Phase A waits for a chain of dependent box reads, so a
    // visit reads as much as one aligned line pair gives: the boxes of all four GRANDCHILDREN of an internal node
    // (heap order: nodes 4n..4n+3, 128 contiguous bytes) -- a grandchild the ball cuts implies its parent is cut,
    // so the level between needs no test of its own.  Which grandchildren are still to be visited is kept as a
    // 4-bit mask per pair of levels; no box is fetched twice.  An odd last level is a two-child visit.
    if (!(box_dist2(pm.tbox + 2, wx, wy, wz) < wr2)) return nl;
    if (n_leaves == 1) { list_leaf(0u); return nl; }
    uint32_t node = wstart;                 // current internal node (the root, or the cell's start node: even depth) ...
    uint32_t pd = (31u - (uint32_t)__clz((int)node)) >> 1;      // ... and its pair-depth (tree depth = 2 * pd)
    uint32_t todo_mask = 0;                 // nibble pd: grandchildren of the path's node at pair-depth pd still to visit (at most 65536 leaves: 8 nibbles)
    for (;;) {
        if (4u * node < 2u * n_leaves && 2u * node < n_leaves) {
            // grandchildren exist (they are internal nodes, or the leaves themselves)
            const float4 *gb = pm.tbox + 8 * (size_t)node + (upper ? 4 : 0);      // boxes of 4*node .. 4*node + 3: two of them for me
            uint32_t m2 = 0;
            if (box_dist2(gb, wx, wy, wz) < wr2) m2 |= 1u;
            if (box_dist2(gb + 2, wx, wy, wz) < wr2) m2 |= 2u;
            const uint32_t m4 = both_halves(m2, 2);
            if (4u * node >= n_leaves) {     // the grandchildren are leaves
                for (int i = 0; i < 4; i++) if ((m4 >> i) & 1u) list_leaf(4u * node + (uint32_t)i - n_leaves);
            } else if (m4) {
                const uint32_t i = (uint32_t)__ffs((int)m4) - 1u;
                todo_mask |= (m4 & ~(1u << i)) << (4u * pd);
                node = 4u * node + i; pd++;
                continue;
            }
        } else {
            // one level left: the children are leaves
            const float4 *cb = pm.tbox + 4 * (size_t)node + (upper ? 2 : 0);
            const uint32_t m2 = both_halves(box_dist2(cb, wx, wy, wz) < wr2 ? 1u : 0u, 1);
            if (m2 & 1u) list_leaf(2u * node - n_leaves);
            if (m2 & 2u) list_leaf(2u * node + 1u - n_leaves);
        }
        if (!todo_mask) break;
        const uint32_t bit = 31u - (uint32_t)__clz((int)todo_mask);            // deepest pair-depth with work left
        const uint32_t d = bit >> 2;
        const uint32_t nib = (todo_mask >> (4u * d)) & 15u;
        const uint32_t i = (uint32_t)__ffs((int)nib) - 1u;                    // its leftmost grandchild not yet visited
        todo_mask &= ~(1u << (4u * d + i));
        node = ((node >> (2u * (pd - d))) << 2) + i;                          // that ancestor's grandchild i
        pd = d + 1u;
    }
    return nl;
}

// ------------------------------------------------------------------------------------------------
// phase B: the wave takes the pending queries one by one
// ------------------------------------------------------------------------------------------------
// query `ql` (the lane that holds it) with its current trial radius, as scalars
__device__ __forceinline__ GatherQuery broadcast_query(const LaneQuery &q, int ql)
{
    GatherQuery Q;
    Q.px = lane_f(q.a.x, ql); Q.py = lane_f(q.a.y, ql); Q.pz = lane_f(q.a.z, ql);
    Q.nx = lane_f(q.a.w, ql); Q.ny = lane_f(q.b.x, ql); Q.nz = lane_f(q.b.y, ql);
    Q.rq2 = lane_f(q.r2cur, ql);
    Q.kscale = 16777000.0f / Q.rq2;            // 24-bit fixed-point distance key (see cand_key)
    return Q;
}

// one more sub-leaf after the real ones, every slot empty: pads a list to whole steps
__device__ __forceinline__ uint32_t dummy_sub(const DevPhotonMap &pm) { return pm.n_leaves * RT_LEAF_SUBS; }

// Test the box of EVERY sub-leaf of the map against the query ball, 64 per step: g(sub-leaf of this lane, whether the ball cuts
// it, the lanes where it does) is called wave-uniformly.  This is the slow path's only way to its sub-leaves (no list is
// kept): its count and each of its passes go through here.
template <class Fn>
__device__ __forceinline__ void scan_all_subboxes(const QueryPass &P, Fn &&g)
{
    const uint32_t n_sub_total = P.pm.n_leaves * RT_LEAF_SUBS;
    for (uint32_t base = 0; base < n_sub_total; base += 64u) {
        const uint32_t sub = base + (uint32_t)P.lane;
        const float bd = sub < n_sub_total ? box_dist2(P.pm.sbox + 2 * (size_t)sub, P.Q.px, P.Q.py, P.Q.pz) : __builtin_inff();
        g(sub, bd < P.Q.rq2, ballot64(bd < P.Q.rq2));
    }
}

// The query's sub-leaves: RT_LEAF_SUBS boxes per listed leaf, tested 64 at a time, the ids of those the ball cuts compacted in
// L.subs.  A leaf holds 128 photon slots and most query balls cut only part of one: its RT_LEAF_SUBS (8) sub-boxes of
// RT_SUB_PHOTONS (16) slots spare the rest.  (Measured when sub-leaves came in, 32 slots each then: about a fifth fewer
// photons examined than with whole 64-slot leaves.)  ql: the lane that holds the query, qnl: the leaves its walk counted.
__device__ __forceinline__ void compact_subleaves(QueryPass &P, int ql, uint32_t qnl)
{
    uint32_t n_sub = 0;
    P.slow = qnl > RT_LEAFLIST_CAP;            // the LDS list overflowed
    wave_sync();                               // the previous query's passes are done with L.subs
    if (P.slow) {
        // list too long for LDS: every pass walks ALL sub-leaf boxes instead (for_each_candidate); here they are only counted
        scan_all_subboxes(P, [&](uint32_t, bool, unsigned long long m) { n_sub += (uint32_t)__popcll(m); });
    } else {
        for (uint32_t base = 0; base < qnl * RT_LEAF_SUBS; base += 64u) {
            const uint32_t e = base + (uint32_t)P.lane;
            const bool have_e = (e / RT_LEAF_SUBS) < qnl;
            const uint32_t sub = have_e ? (uint32_t)P.L.leaves[ql][e / RT_LEAF_SUBS] * RT_LEAF_SUBS + (e % RT_LEAF_SUBS) : 0u;
            const float bd = have_e ? box_dist2(P.pm.sbox + 2 * (size_t)sub, P.Q.px, P.Q.py, P.Q.pz) : __builtin_inff();
            const unsigned long long m = ballot64(bd < P.Q.rq2);
            if (bd < P.Q.rq2) P.L.subs[n_sub + lanes_below(m)] = sub;
            n_sub += (uint32_t)__popcll(m);
        }
        if (P.lane < RT_SUBS_PER_STEP) P.L.subs[n_sub + P.lane] = dummy_sub(P.pm);
        wave_sync();
    }
    P.n_sub = n_sub;
}

// One pass over the photons of the query's sub-leaves: f(candidate, byte offset of its slot), wave-uniformly (scan_subleaves).
// The slow path lists the sub-leaves of one step of scan_all_subboxes at a time.
template <class F>
__device__ __forceinline__ void for_each_candidate(const QueryPass &P, F &&f)
{
    if (!P.slow) { scan_subleaves(P.pm, P.L.subs, P.n_sub, P.lane, P.Q, f); return; }
    scan_all_subboxes(P, [&](uint32_t sub, bool cut, unsigned long long m) {
        if (!m) return;
        wave_sync();
        if (cut) P.L.subs[lanes_below(m)] = sub;
        const uint32_t cnt = (uint32_t)__popcll(m);
        if (P.lane < RT_SUBS_PER_STEP) P.L.subs[cnt + P.lane] = dummy_sub(P.pm);
        wave_sync();
        scan_subleaves(P.pm, P.L.subs, cnt, P.lane, P.Q, f);
    });
}

// "Sparse here": the cell's last query found no more than k photons inside the FULL radius.  Then all accepted
// photons count and dist2[0] stays radius^2 (cyPhotonMap.h:309-326): one plain pass sums them -- no histogram, no ring,
// no selection.  Returns the number of accepted photons; if that is more than k after all, the caller drops the sums and
// takes the normal path.
__device__ __forceinline__ uint32_t sparse_pass(const QueryPass &P, GatherSums &s)
{
    const float rq2 = P.Q.rq2;
    uint32_t M = 0;
    for_each_candidate(P, [&](const Cand &cd, uint32_t) {
        M += (uint32_t)__popcll(ballot64(cd.d2 < rq2));
        if (cd.d2 < rq2) s.add(cd.pa, cd.pb);
    });
    return M;
}

// The band the k-th squared distance is expected in, around the prediction: the cell's memory, else this wave's previous
// query, else the first radius' own assumption (RT_GATHER_GUESS * k photons inside rq2).
__device__ __forceinline__ GatherBand predict_band(float pred_rk2, float rq2, bool final_round)
{
    const float pk = (pred_rk2 > 0.0f && pred_rk2 < rq2) ? pred_rk2 : rq2 * (1.0f / RT_GATHER_GUESS);
    GatherBand B;
    B.t_lo = RT_GATHER_BAND_LO * pk;
    B.t_hi = final_round ? rq2 : fminf(RT_GATHER_BAND_HI * pk, rq2);     // <= rq2: inside the band implies accepted
    return B;
}

// Pass 1: count + histogram of every accepted photon.  Photons closer than t_lo (safely inside the k nearest if the
// prediction holds) are summed right away; those between t_lo and t_hi, the band the k-th distance is expected in, are
// parked in the LDS ring with all their data.  M: accepted photons (wave-uniform: popcount of the ballots).  Returns the
// number of photons in the band (wave-uniform too); those past RT_GATHER_RING were not kept.
__device__ __forceinline__ uint32_t pass1(const QueryPass &P, const GatherBand &B, GatherSums &s, uint32_t &M)
{
    GatherLds &L = P.L;
    const float rq2 = P.Q.rq2, t_lo = B.t_lo, t_hi = B.t_hi;
    *(uint4 *)&L.hist[4 * P.lane] = make_uint4(0u, 0u, 0u, 0u);     // the 256 bins in one 16-byte store per lane
    wave_sync();
    // The histogram bin is the top 8 bits of the 24-bit key: (uint)(d2 * kscale) >> 16 == (uint)(d2 * (kscale / 65536)),
    // the scaling by a power of two being exact.
    const float kscale_bin = P.Q.kscale * (1.0f / 65536.0f);
    uint32_t n_ring = 0;
    for_each_candidate(P, [&](const Cand &cd, uint32_t) {
        const unsigned long long m_ok = ballot64(cd.d2 < rq2);
        const unsigned long long m_lo = ballot64(cd.d2 < t_lo);
        const unsigned long long mr = ballot64(cd.d2 < t_hi) & ~m_lo;
        M += (uint32_t)__popcll(m_ok);
        if (cd.d2 < rq2) atomicAdd(&L.hist[(uint32_t)(cd.d2 * kscale_bin)], 1u);
        if (cd.d2 < t_lo) s.add(cd.pa, cd.pb);
        if (mr) {
            if (cd.d2 < t_hi && !(cd.d2 < t_lo)) {
                const uint32_t at = n_ring + lanes_below(mr);
                if (at < (uint32_t)RT_GATHER_RING) {
                    L.ring_a[at] = make_float4(cd.d2, cd.pa.w, cd.pb.x, cd.pb.y);
                    L.ring_b[at] = make_float2(cd.pb.z, cd.pb.w);
                }
            }
            n_ring += (uint32_t)__popcll(mr);
        }
    });
    return n_ring;
}

// Locate the K-th smallest key among the accepted photons, from pass 1's histogram: 8 bits of the key per level, until
// the bin that holds it has at most 64 photons (or the key has no bits left: more than 64 photons with identical keys).
__device__ __forceinline__ KthBin locate_kth(const QueryPass &P, uint32_t K)
{
    GatherLds &L = P.L;
    const int lane = P.lane;
    KthBin kb = {K, 0u, 0u, 16};
    for (;;) {
        wave_sync();
        const uint4 h4 = *(const uint4 *)&L.hist[4 * lane];
        const uint32_t h0 = h4.x, h1 = h4.y, h2 = h4.z, h3 = h4.w;
        const uint32_t mine = h0 + h1 + h2 + h3;
        const uint32_t incl = wave_scan_add_u(mine);
        const uint32_t excl = incl - mine;
        const unsigned long long m = ballot64(incl >= kb.need);
        const int owner = __ffsll((long long)m) - 1;      // first lane whose range reaches `need`
        uint32_t digit = 0, before = 0, cntb = 0;
        if (lane == owner) {
            const uint32_t cum = excl;
            if (cum + h0 >= kb.need) { digit = 4 * lane; before = cum; cntb = h0; }
            else if (cum + h0 + h1 >= kb.need) { digit = 4 * lane + 1; before = cum + h0; cntb = h1; }
            else if (cum + h0 + h1 + h2 >= kb.need) { digit = 4 * lane + 2; before = cum + h0 + h1; cntb = h2; }
            else { digit = 4 * lane + 3; before = cum + h0 + h1 + h2; cntb = h3; }
        }
        digit = lane_u(digit, owner); before = lane_u(before, owner); cntb = lane_u(cntb, owner);
        kb.need -= before;
        kb.prefix |= digit << kb.shift;
        kb.in_bin = cntb;
        if (kb.in_bin <= 64u || kb.shift == 0) break;
        // one more level: histogram of the next 8 bits over the photons inside this bin
        kb.shift -= 8;
        wave_sync();
        *(uint4 *)&L.hist[4 * lane] = make_uint4(0u, 0u, 0u, 0u);
        wave_sync();
        const uint32_t hi_mask = ~((1u << (kb.shift + 8)) - 1u) & 0xFFFFFFu;
        const uint32_t prefix = kb.prefix; const int shift = kb.shift;
        for_each_candidate(P, [&](const Cand &cd, uint32_t) {
            const uint32_t key = cand_key(cd, P.Q);
            if (cd.d2 < P.Q.rq2 && (key & hi_mask) == prefix) atomicAdd(&L.hist[(key >> shift) & 255u], 1u);
        });
    }
    return kb;
}

// The ring serves the selection when (1) it did not overflow, (2) the k-th photon's bin was resolved at the first level,
// (3) every photon below t_lo lies in an earlier bin (so all of them count) and (4) every photon of the k-th bin or earlier
// lies below t_hi (so it is either summed already or in the ring).  Keys are monotone in d2, which makes (3) and (4) exact.
__device__ __forceinline__ bool ring_serves(const GatherQuery &Q, const GatherBand &B, const KthBin &kb, uint32_t n_ring)
{
    const uint32_t bin_lo = (uint32_t)(B.t_lo * Q.kscale) >> 16, bin_hi = (uint32_t)(B.t_hi * Q.kscale) >> 16;
    const uint32_t kbin = kb.prefix >> 16;
    return kb.shift == 16 && kb.in_bin <= 64u && n_ring <= (uint32_t)RT_GATHER_RING && bin_lo < kbin && (B.t_hi >= Q.rq2 || kbin < bin_hi);
}

// Selection without a second read of the leaves: of the ring's photons, those in bins before the k-th's are summed (the ones
// below t_lo were in pass 1), those of the k-th bin go to the selection list (d2, ring index).
__device__ __forceinline__ void collect_from_ring(const QueryPass &P, const KthBin &kb, uint32_t n_ring, GatherSums &s)
{
    GatherLds &L = P.L;
    const uint32_t bin_mask = kb.mask();
    for (uint32_t base = 0; base < n_ring; base += 64u) {
        const uint32_t idx = base + (uint32_t)P.lane;
        const bool have = idx < n_ring;
        const float4 ra = have ? L.ring_a[idx] : make_float4(3.0e38f, 0, 0, 0);
        const float2 rb = have ? L.ring_b[idx] : make_float2(0, 0);
        const uint32_t kbits = (uint32_t)(ra.x * P.Q.kscale) & bin_mask;
        const bool take = have && kbits < kb.prefix;
        const bool inb = have && kbits == kb.prefix;
        const unsigned long long mb = ballot64(inb);
        if (mb) {
            const uint32_t sbase = lane_u(L.sel_n, 0);
            if (inb) {
                const uint32_t at = sbase + lanes_below(mb);
                if (at < 64u) { L.sel_d[at] = ra.x; L.sel_i[at] = idx; }
            }
            wave_sync();
            if (P.lane == 0) L.sel_n = sbase + (uint32_t)__popcll(mb);
            wave_sync();
        }
        if (take) s.add(ra.y, ra.z, ra.w, rb.x, __float_as_uint(rb.y));
    }
}

// Pass 2, when the ring does not serve: the sums start over; everything in bins before the k-th's is summed and that bin's
// photons go to the selection list (d2, byte offset of the slot).  If more than 64 photons share all 24 key bits there is no
// list: the first `need` of them in scan order are taken here, tmax = the largest distance this lane took.
__device__ __forceinline__ void pass2(const QueryPass &P, const KthBin &kb, GatherSums &s, float &tmax)
{
    GatherLds &L = P.L;
    const float rq2 = P.Q.rq2;
    const uint32_t bin_mask = kb.mask();
    uint32_t tie_taken = 0;                // only used when in_bin > 64 (identical keys)
    s.clear();
    for_each_candidate(P, [&](const Cand &cd, uint32_t slot) {
        const bool ok = cd.d2 < rq2;
        const uint32_t kbits = cand_key(cd, P.Q) & bin_mask;
        bool take = ok && kbits < kb.prefix;
        const bool inb = ok && kbits == kb.prefix;
        const unsigned long long mb = ballot64(inb);
        if (kb.in_bin <= 64u) {
            if (mb) {
                uint32_t base = 0;
                const int leader = __ffsll((long long)mb) - 1;
                if (P.lane == leader) { base = L.sel_n; L.sel_n = base + (uint32_t)__popcll(mb); }
                base = lane_u(base, leader);
                if (inb) {
                    const uint32_t at = base + lanes_below(mb);
                    if (at < 64u) { L.sel_d[at] = cd.d2; L.sel_i[at] = slot; }
                }
            }
        } else {
            const uint32_t rank = tie_taken + lanes_below(mb);
            if (inb && rank < kb.need) { take = true; tmax = fmaxf(tmax, cd.d2); }
            tie_taken += (uint32_t)__popcll(mb);
        }
        if (take) s.add(cd.pa, cd.pb);
    });
}

// Exact selection from the list (at most 64 entries, one per lane): rank by (d2, list position); ranks < need are taken.
// An entry names its photon by ring index (from_ring) or by the byte offset of its slot.
__device__ __forceinline__ void select_ranked(const QueryPass &P, uint32_t need, bool from_ring, GatherSums &s, float &tmax)
{
    const GatherLds &L = P.L;
    const uint32_t n_sel = lane_u(min(L.sel_n, 64u), 0);
    const bool mine = (uint32_t)P.lane < n_sel;
    const float md = mine ? L.sel_d[P.lane] : 3.0e38f;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n_sel; j++) {
        const float od = L.sel_d[j];
        rank += (od < md || (od == md && j < (uint32_t)P.lane)) ? 1u : 0u;
    }
    if (mine && rank < need) {
        const uint32_t si = L.sel_i[P.lane];
        float4 pa, pb;                             // the photon as its slot holds it (position not needed)
        if (from_ring) {
            const float4 ra = L.ring_a[si]; const float2 rb = L.ring_b[si];
            pa = make_float4(0, 0, 0, ra.y); pb = make_float4(ra.z, ra.w, rb.x, rb.y);
        } else { pa = *(const float4 *)((const char *)P.pm.pa + si); pb = *(const float4 *)((const char *)P.pm.pb + si); }
        s.add(pa, pb);                             // one add for both sources: its multiplies and adds stay together and fuse
        tmax = md;
    }
}

// More than K photons inside the radius: sum exactly the K nearest.  Returns np.dist2[0], the largest distance kept.
// n_reads counts a second read of the sub-leaves when the ring could not serve.
__device__ __forceinline__ float select_k_nearest(const QueryPass &P, const GatherBand &B, uint32_t K, uint32_t n_ring, GatherSums &s, uint32_t &n_reads)
{
    GatherLds &L = P.L;
    const KthBin kb = locate_kth(P, K);
    wave_sync();                           // the histogram is dead from here on: its LDS now holds the selection
    if (P.lane == 0) L.sel_n = 0;
    wave_sync();
    float tmax = 0.0f;
    const bool from_ring = ring_serves(P.Q, B, kb, n_ring);
    if (from_ring) collect_from_ring(P, kb, n_ring, s);
    else { n_reads += P.n_sub; pass2(P, kb, s, tmax); }
    wave_sync();
    if (kb.in_bin <= 64u) select_ranked(P, kb.need, from_ring, s, tmax);
    return wave_max0(tmax);
}

// At most k inside the full radius: all of them count.  Pass 1 summed those below t_lo and, in the final round, parked
// every other one in the ring; if that overflowed, sum them with one more pass.
__device__ __forceinline__ void sum_all_accepted(const QueryPass &P, uint32_t n_ring, GatherSums &s, uint32_t &n_reads)
{
    if (n_ring <= (uint32_t)RT_GATHER_RING) {
        for (uint32_t base = 0; base < n_ring; base += 64u) {
            const uint32_t idx = base + (uint32_t)P.lane;
            if (idx < n_ring) {
                const float4 ra = P.L.ring_a[idx];
                const float2 rb = P.L.ring_b[idx];
                s.add(ra.y, ra.z, ra.w, rb.x, __float_as_uint(rb.y));
            }
        }
    } else {
        n_reads += P.n_sub;
        s.clear();
        for_each_candidate(P, [&](const Cand &cd, uint32_t) { if (cd.d2 < P.Q.rq2) s.add(cd.pa, cd.pb); });
    }
}

// The query is done: its six sums and r_k^2 go to ITS lane; what follows from them (area, normalisation, the
// weighted add into the sample) is the same scalar arithmetic for every query, so it is done for all the
// queries a round finished at once, one per lane, in finish_queries -- not 64 lanes wide per query.
__device__ __forceinline__ void deliver(LaneQuery &q, int lane, int ql, const GatherSums &s, uint32_t M, float area_d2)
{
    float t[6];
    wave_sum6(s.pr, s.pg, s.pb, s.dx, s.dy, s.dz, t);
    if (lane == ql) {
        q.f_pr = t[0]; q.f_pg = t[1]; q.f_pb = t[2]; q.f_dx = t[3]; q.f_dy = t[4]; q.f_dz = t[5];
        q.f_area = M > 0 ? area_d2 : -1.0f;      // dist2[0] >= 0; negative: no photon at all
        q.finish = true;
        q.pending = false;
    }
}

// Every lane whose query a round finished: area, normalisation, the output of the launch's mode, and what the query's
// cell remembers for the next one.
template <bool FX>
__device__ __forceinline__ void finish_queries(const GatherArgs &G, LaneQuery &q, float r2)
{
    if (!q.finish) return;
    float irr_r = q.f_pr, irr_g = q.f_pg, irr_b = q.f_pb, dx = q.f_dx, dy = q.f_dy, dz = q.f_dz;
    // remember the k-th distance for the next query of this cell (only when more than k qualified: f_area < r2)
    // (or that no more than k were inside the full radius: f_area is then radius^2, or negative without any photon)
    if (G.cell_rk2 && G.pm.n_leaves > 1) {
        if (q.f_area > 0.0f && q.f_area < r2) G.cell_rk2[q.cell_index] = q.f_area;
        else if (q.r2cur >= r2) G.cell_rk2[q.cell_index] = -1.0f;
    }
    if (q.f_area >= 0.0f) {
        const float area = (float)M_PI * q.f_area;             // :326
        if (area > 0) { const float inv = 1.0f / area; irr_r *= inv; irr_g *= inv; irr_b *= inv; }
        const float l = sqrtf(dx * dx + dy * dy + dz * dz);    // direction.Normalize() :334
        dx /= l; dy /= l; dz /= l;
    }
    if (G.mode == 1) {
        const size_t qq = (size_t)q.qi;
        G.out_irr[3 * qq] = irr_r; G.out_irr[3 * qq + 1] = irr_g; G.out_irr[3 * qq + 2] = irr_b;
        G.out_dir[3 * qq] = dx; G.out_dir[3 * qq + 1] = dy; G.out_dir[3 * qq + 2] = dz;
    } else {
        // idr_Color += kd * photonrad * max(0, N.(-dir)) (FIN/main.cpp:701-704), times the ray weight
        const float nx = q.a.w, ny = q.b.x, nz = q.b.y, wr = q.b.z, wg = q.b.w, wb = q.c.x;
        const uint32_t slot = __float_as_uint(q.c.y);
        float theta = nx * (-dx) + ny * (-dy) + nz * (-dz);
        theta = theta > 0.0f ? theta : 0.0f;
        if constexpr (FX) fx_add(G.fx + 3 * (size_t)slot, (wr * irr_r) * theta, (wg * irr_g) * theta, (wb * irr_b) * theta);
        else {
            float *dst = G.sample_rgb + 3 * (size_t)slot;
            atomicAdd(dst, (wr * irr_r) * theta);
            atomicAdd(dst + 1, (wg * irr_g) * theta);
            atomicAdd(dst + 2, (wb * irr_b) * theta);
        }
    }
    q.finish = false;
}

// The wave's tallies into the launch's statistics: a workgroup adds its counters up in LDS and ONE thread per counter
// flushes them (flush_counters in rt_shade.h says why).  Workgroup-uniform; every wave of the workgroup gets here.
__device__ __forceinline__ void flush_gather_stats(const GatherArgs &G, int lane, const GatherTally &T, uint32_t nq)
{
    if (!G.stats) return;
    __shared__ unsigned long long s_acc[4];
    if (threadIdx.x < 4) s_acc[threadIdx.x] = 0;
    __syncthreads();
    if (lane == 0 && T.visited) {
        atomicAdd(&s_acc[0], T.visited * (unsigned long long)RT_SUB_PHOTONS);
        atomicAdd(&s_acc[1], (unsigned long long)T.n_rounds);
        atomicAdd(&s_acc[2], (unsigned long long)T.n_slow);
        atomicAdd(&s_acc[3], (unsigned long long)T.n_reads * RT_SUB_PHOTONS / 32ull);     // in units of 32 slots = 1 KiB
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int slot = threadIdx.x == 0 ? ST_PHOTONS_VISITED : threadIdx.x == 1 ? ST_GATHER_ROUNDS : threadIdx.x == 2 ? ST_GATHER_SLOW : ST_GATHER_LEAF_READS;
        const unsigned long long x = s_acc[threadIdx.x];
        if (x) atomicAdd(&G.stats[ST_AT(slot)], x);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&G.stats[ST_AT(ST_PHOTON_QUERIES)], (unsigned long long)nq);
}

#ifndef RT_GATHER_WAVES_PER_EU
#define RT_GATHER_WAVES_PER_EU 5     // 96 registers: five waves per SIMD is what the LDS footprint allows too
#endif
template <bool FX = false>
__attribute__((amdgpu_waves_per_eu(RT_GATHER_WAVES_PER_EU, RT_GATHER_WAVES_PER_EU)))
__global__ __launch_bounds__(64 * RT_GATHER_WAVES) void k_gather(GatherArgs G)
{
    __shared__ GatherLds lds_all[RT_GATHER_WAVES];
    GatherLds &L = lds_all[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    uint32_t nq = *G.count_ptr;
    if (nq > G.count_cap) nq = G.count_cap;
    if (nq == 0) return;                                 // most chunks of a frame see no photon query at all
    const float r2 = G.radius * G.radius;
    const uint32_t K = (uint32_t)G.k;
    GatherTally T = {0ull, 0u, 0u, 0u};
    float pred_rk2 = 0.0f;                                // k-th squared distance of this wave's previous query (a hint only)
    const uint32_t n_batches = (nq + (uint32_t)RT_GATHER_BATCH - 1u) / (uint32_t)RT_GATHER_BATCH;
    const float guess_c = RT_GATHER_GUESS * (float)K * G.pm.cell * G.pm.cell / (float)M_PI;

    uint32_t seg = home_segment();
    for (uint32_t qbase; (qbase = claim_batch(G, lane, n_batches, seg)) != RT_GATHER_NO_BATCH;) {
        LaneQuery q = load_query(G, lane, qbase, nq);
        first_radius(G, q, r2, guess_c);
        while (ballot64(q.pending)) {
            const uint32_t nl = list_leaves(G.pm, L, lane, q);                  // phase A
            wave_sync();
            for (unsigned long long todo = ballot64(q.pending); todo; todo &= todo - 1) {      // phase B
                const int ql = __ffsll((long long)todo) - 1;
                QueryPass P = {G.pm, L, lane, broadcast_query(q, ql), false, 0u};
                const float rq2 = P.Q.rq2;
                const bool final_round = rq2 >= r2;
                compact_subleaves(P, ql, lane_u(nl, ql));
                T.n_rounds++; T.n_slow += P.slow ? 1u : 0u; T.n_reads += P.n_sub;

                GatherSums s; s.clear();
                uint32_t M = 0;                            // accepted photons
                float area_d2 = rq2;                       // dist2[0]: stays the full radius^2 when at most k qualify
                const float cell_pred = lane_f(q.cell_pred, ql);
                bool sparse = final_round && cell_pred < 0.0f;
                if (sparse) {
                    M = sparse_pass(P, s);
                    T.visited += P.n_sub;
                    if (M > K) { sparse = false; M = 0; s.clear(); T.n_reads += P.n_sub; }      // not sparse after all
                }
                if (!sparse) {
                    if (cell_pred > 0.0f) pred_rk2 = cell_pred;
                    const GatherBand B = predict_band(pred_rk2, rq2, final_round);
                    const uint32_t n_ring = pass1(P, B, s, M);
                    T.visited += P.n_sub;
                    if (!final_round && M <= K) {
                        // not enough inside the trial radius: grow it (count ~ r^2 on a surface) and retry
                        float grow = 1.5f * (float)K / (float)(M > 0 ? M : 1u);
                        grow = fminf(fmaxf(grow, 2.0f), 16.0f);
                        if (lane == ql) q.r2cur = fminf(rq2 * grow, r2);
                        continue;
                    }
                    if (M > K) pred_rk2 = area_d2 = select_k_nearest(P, B, K, n_ring, s, T.n_reads);
                    else if (M > 0) sum_all_accepted(P, n_ring, s, T.n_reads);
                }
                deliver(q, lane, ql, s, M, area_d2);
            }
            finish_queries<FX>(G, q, r2);
            wave_sync();
        }
    }
    flush_gather_stats(G, lane, T, nq);
}

void rtk_launch_gather(hipStream_t st, const GatherRequest &R, int blocks)
{
    GatherArgs G; G.pm = R.pm; G.cell_rk2 = R.cell_rk2; G.fx = R.fx; G.qa = R.q.qa; G.qb = R.q.qb; G.qc = R.q.qc; G.count_ptr = R.count; G.count_cap = R.q.cap;
    G.k = R.k; G.radius = R.radius; G.sample_rgb = R.sample_rgb; G.out_irr = R.out_irr; G.out_dir = R.out_dir; G.mode = R.out_irr ? 1 : 0;
    G.stats = R.stats; G.next_batch = R.next_batch;
    if (G.fx && G.mode == 0) hipLaunchKernelGGL(k_gather<true>, dim3(blocks), dim3(64 * RT_GATHER_WAVES), 0, st, G);
    else hipLaunchKernelGGL(k_gather<false>, dim3(blocks), dim3(64 * RT_GATHER_WAVES), 0, st, G);
}
