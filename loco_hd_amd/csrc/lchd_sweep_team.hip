// lchd_sweep_team.hip -- K2 for the pairs that fit ONE tile, several per wavefront: k_sweep_duo<CMAX, TL, TILE, WGT, KSM> stages the
// two environments of every pair of a wavefront and runs the team tile (lchd_team_tile.h) -- LoCoHD::stat_dist_integral,
// /root/reference/src/locohd.rs:61-226, for Hellinger-2 (unit or weighted categories) and Kolmogorov-Smirnov.
#include "lchd_sweep_common.h"

namespace lchd {
// What a pair record means to the team kernel of `rule` -- for the batch's sort key and for the iteration that sweeps the pair alike.
struct TeamPair {
    int nA, nB;   // points of the two environments, anchors included
    bool mine;    // this kernel writes the pair's score: it sweeps it, or the pair is unusable (NaN); larger pairs belong to k_sweep
    bool valid;   // this kernel sweeps it
};
__device__ __forceinline__ TeamPair team_pair(int rule, bool live, const int4& m) {
    TeamPair k;
    k.nA = m.z & 0xFFFFFF;
    k.nB = m.w & 0xFFFFFF;
    const bool usable = live && k.nA > 0 && k.nB > 0;
    k.mine = !usable || pair_is_small(rule, k.nA, k.nB);
    k.valid = usable && k.mine;
    return k;
}
// The stable rank of a lane's key (0 .. 15) among the first kb lanes of the wavefront; a lane beyond them keeps its own number, so the
// ranks are a permutation of 0 .. 63.  A 4-bit radix over ballots, most significant bit first: every lane keeps the set of lanes whose
// key is smaller than its own (lt) and of those that agree with it in the bits seen so far (eq); its rank is |lt| + the lanes of eq
// before it.  A pure function of the keys (no atomics): the same list always gets the same co-scheduling.  (Sixteen ballot + mbcnt
// steps, one per key value, come out 13 vector instructions longer.)
__device__ __forceinline__ int team_batch_rank(int key, int lane, int kb) {
    const bool inb = lane < kb;
    uint64_t lt = 0ull, eq = __ballot(inb);
#pragma unroll
    for (int bit = 3; bit >= 0; --bit) {
        const bool one = (key >> bit) & 1;
        const uint64_t b = __ballot(one);
        lt |= one ? (eq & ~b) : 0ull;
        eq &= one ? b : ~b;
    }
    const int r = __popcll(lt) + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(eq >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)eq, 0u));
    return inb ? r : lane;
}

// ------------------------------------------------------------------------------------------------
// K2 for small environments: TWO (or four) anchor pairs per wavefront and iteration, 32 (16) lanes each.
//
// With environments of ~70-100 points per side (coarse-grained typing, the reference's main use) a pair has ~150 merged
// events: one wavefront per pair spends most of its instructions on the per-tile prologue (staging, merge path, scan, state
// reload, reduction), all of them executed for 64 lanes of which a third idle.  Here every wave-wide instruction serves two
// pairs.  A pair qualifies if it has at most kDuoTile merged events (exactly one tile, no carries between tiles); the
// configuration must be Hellinger-2 with unit category weights, CDF-keyed environments, at most 16 category slots.  The
// host launches this kernel AND k_sweep; k_pair_meta counts the qualifying pairs (DeviceStatus::n_small): when they are
// the majority this kernel sweeps them and k_sweep only the rest, otherwise this kernel returns at once.
//
// Batches.  The tile's loops run a wave-uniform number of trips, the longest chunk length epl = ceil(T / TL) among the wavefront's
// teams; a team with a shorter chunk issues the other trips with its lanes masked off.  So a wavefront does not take TEAMS consecutive
// pairs per iteration but a BATCH of `batch` consecutive pairs (a kernel argument, at most 64, a multiple of TEAMS; grid-stride over
// batches): once per batch every lane loads ONE pair record (coalesced), works out its key -- epl if this kernel sweeps the pair, else
// 0 -- and its stable rank among the batch's keys (team_batch_rank); one ds_permute sends the lane's number to the lane of its rank.
// Iteration q sweeps the pairs of rank TEAMS q + team: a ds_bpermute fetches the pair's place in the batch, the record is read again
// (from the cache) and everything per pair -- out[p], wf_index[p], offsets, anchors' categories -- follows that p.  Teams of equal
// chunk length share a wavefront; the pairs of key 0 come first and an iteration without a pair to sweep is skipped (its unusable
// pairs get their NaN).  Only the record's PLACE is kept in a register across the tile (one VGPR: the 28-slot form stands at its limit
// of 168), and no LDS is added.  A pair's score does not depend on its partners: the trip counts only bound loops whose bodies are
// guarded per lane.
// ------------------------------------------------------------------------------------------------
constexpr int kTeamBigWaves = 3;   // waves per SIMD k_sweep_duo is compiled for with more than 16 category slots, and with category weights and 9 .. 16 (their counts in LDS bytes, TeamTile::LCNT); 4 otherwise
// (the name is historic: round 1 swept TWO pairs per wavefront; with TL = 16 a wavefront sweeps FOUR -- the per-tile prologue, which
// is two thirds of this kernel's instructions at ~150 events per pair, is shared by twice as many pairs, the event loop costs the
// same per pair: C3 459 -> see DESIGN section 4)
// TILE_ = 240: pairs of at most 240 merged events (small_rule 0); TILE_ = 480 (TL = 32): pairs whose environments both have at most
// 255 points and that have at most 480 merged events (small_rule 2) -- the 8-bit-count k_sweep's pairs, two per wavefront (C2a: ~343
// events per pair)
// WGT: category weights other than 1 (pmf.rs:47-63 adds weight[c] per point): H^2 = 1 - sum_c w_c sqrt(a_c b_c) / sqrt(W_a W_b) with the
// weighted totals W = sum_c w_c count_c -- the same integer count fields and tables, one multiplier per category from LDS, two
// running totals and one reciprocal square root per event instead of the two table look-ups of the unit-weight form.
// KSM: the Kolmogorov-Smirnov distance max_c |a_c / N_a - b_c / N_b| (statistical_distances.rs:12-21) with unit weights instead of
// Hellinger-2: every event needs all categories, but as INTEGERS -- max_c |a_c N_b - b_c N_a| over the 8-bit count fields (two 24-bit
// multiplies, one v_sad_u32, one max per category), scaled once by 1 / (N_a N_b) from the reciprocal-root table; no square root.
template <int CMAX, int TL = kDuoTL, int TILE_ = kDuoTile, bool WGT = false, bool KSM = false, bool PRE = false>
__global__ __launch_bounds__(64 * kSweepWaves, ((CMAX <= 16 && !(WGT && CMAX > 8)) ? 4 : kTeamBigWaves)) void k_sweep_duo(SweepArgs args, int batch) {
    // (the tile itself -- merge path, chunk histogram, count scans, event loop, stitching -- is lchd_team_tile.h)
    using TT = TeamTile<CMAX, TL, TILE_, WGT, KSM, PRE>;
    constexpr int TEAMS = TT::TEAMS, EPL = TT::EPL, TILE = TT::TILE, WPB = kSweepWaves, NT = TT::NT, LW = TT::LW;
    constexpr bool LCNT = TT::LCNT;
    constexpr int RULE = TILE_ == kDuoTile ? 0 : 2;
    __shared__ double t_sqrt[NT], t_rsqrt[NT];
    // one buffer per team: list A's points, its sentinel (and a pad entry behind an even list), list B's points, its sentinel: at most
    // TILE points together, list B starts at entry TILE + 2 at most and its sentinel lies at entry TILE + 2 at most (TILE + 4: the teams'
    // buffers stay 16-byte aligned)
    __shared__ uint64_t s_[WPB][TEAMS][TILE + 4];
    __shared__ uint8_t c_[WPB][TEAMS][TILE + 8];
    // (TeamTile's PRE branch reads up to kPreStep - 1 category bytes behind a chunk's start without a clamp: a chunk of list B starts at
    // byte TILE + 2 of a team's row at most, so the reads end at byte TILE + 2 + kPreStep - 1)
    static_assert(!PRE || TILE + 2 + (kPreStep - 1) < TILE + 8, "spare category bytes behind list B for the unclamped reads of the prefix-count rows");
    __shared__ uint64_t lc_[LCNT ? WPB : 1][LCNT ? LW * 64 : 1];  // (TeamTile::LCNT: per-lane count rows of the event loop)
    __shared__ double w_s[WGT ? 32 : 1];
    if (!args.forced && rule_in_force(args) != RULE) return;  // another rule's pairs are the majority, or none's: k_sweep sweeps everything
    const int tid = threadIdx.x, lane = tid & 63, tl = lane & (TL - 1), team = lane / TL;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const DevConfig* __restrict__ cfgp = args.cfg;
    const double Finf0 = cfgp->wf_finf[0];
    for (int k = tid; k < NT; k += 64 * WPB) {
        t_sqrt[k] = args.sqrt_tab[k];
        t_rsqrt[k] = args.rsqrt_tab[k];
    }
    if constexpr (WGT) {
        if (tid < 32) w_s[tid] = tid < cfgp->n_categories ? cfgp->cat_w[tid] : 0.0;
    }
    __syncthreads();
    uint64_t* sA = s_[wv][team];
    uint8_t* cA = c_[wv][team];
    unsigned char* lcl = reinterpret_cast<unsigned char*>(lc_[LCNT ? wv : 0]) + lane * 8;  // this lane's eight bytes of word 0

    // ---- batches: kb consecutive pairs per wavefront, one record per lane, co-scheduled by chunk length (see the header) ----
    const int kb = __builtin_amdgcn_readfirstlane(batch);  // TEAMS <= kb <= 64, a multiple of TEAMS
    const int64_t bstride = (int64_t)gridDim.x * WPB * kb;
    for (int64_t base = ((int64_t)blockIdx.x * WPB + wv) * kb; base < args.n_pairs; base += bstride) {
        int sl;  // lane r: the index in the batch of the pair of rank r (p = base + sl), -1 where the batch has no such pair
        {
            // (the lane number, worked out HERE from a zero the optimiser cannot see through: carried from the kernel's head it is one more
            // register live across the tile, and the 28-slot forms, which stand at their limit of 168, spill it)
            uint32_t zero = 0u;
            asm volatile("" : "+v"(zero));
            const int bl = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero));
            const int nrec = (int)min((int64_t)kb, args.n_pairs - base);  // (wave-uniform) the last batch of the list may be short
            const bool have = bl < nrec;
            const int4 r = (args.meta + base)[have ? bl : 0];
            const TeamPair tp = team_pair(RULE, have, r);
            // the key: the pair's chunk length; 0 for every pair this kernel does not sweep -- they sort together and first
            const int key = tp.valid ? (tp.nA + tp.nB - 2 + TL - 1) / TL : 0;
            // (wave-uniform: a batch of one iteration's pairs -- what a short launch gets -- has nothing to rank)
            const int rank = kb > TEAMS ? team_batch_rank(key, bl, kb) : bl;
            sl = __builtin_amdgcn_ds_permute(rank * 4, have ? bl : -1);
        }
        const int nq = kb / TEAMS;
#pragma unroll 1
        for (int q = 0; q < nq; ++q) {
            const int src = (q * TEAMS + team) * 4;  // this team's pair of the iteration: rank TEAMS q + team
            const int pl = __builtin_amdgcn_ds_bpermute(src, sl);
            const bool live = pl >= 0;
            const int64_t p = base + (live ? pl : 0);
            const int4 m = args.meta[p];  // (the batch's records are in the cache: every lane of the wavefront has just read one)
            const TeamPair tp = team_pair(RULE, live, m);
            const bool mine = tp.mine, valid = tp.valid;
            if (__ballot(valid) == 0ull) {  // (wave-uniform) nothing to sweep: an unusable pair still gets its NaN
                if (tl == TL - 1 && live && mine) args.out[p] = nan("");
                continue;
            }
            const int mA = valid ? tp.nA - 1 : 0, mB = valid ? tp.nB - 1 : 0, T = mA + mB;  // non-anchor events
            const int c0a = (m.z >> 24) & 255, c0b = (m.w >> 24) & 255;
            // (a dictionary's key sets: the set of this pair's weight function -- k_pair_meta has checked the index of every usable pair)
            int64_t ksetA = 0, ksetB = 0;
            if (args.wf_index) {  // (wave-uniform: configurations with one weight function never multiply)
                const int64_t kset = valid ? args.wf_index[p] : 0;
                ksetA = kset * args.env_a.set_stride;
                ksetB = kset * args.env_b.set_stride;
            }
            // (slot x stride as ONE 32 x 32 -> 64-bit multiply: slots and strides are below 2^31)
            const uint64_t offA = (uint64_t)(uint32_t)m.x * (uint32_t)args.env_a.stride, offB = (uint64_t)(uint32_t)m.y * (uint32_t)args.env_b.stride;
            const uint64_t* __restrict__ kA = args.env_a.key + offA + ksetA;
            const uint64_t* __restrict__ kB = args.env_b.key + offB + ksetB;
            const uint8_t* __restrict__ tA = args.env_a.cat + offA;
            const uint8_t* __restrict__ tB = args.env_b.cat + offB;
            const double F0 = valid ? u2d(kA[0]) : 0.0;            // F(0): both anchors sit at distance 0
            // list B starts at an EVEN entry of the buffer behind list A's SENTINEL entry sA[mA] (one entry behind an odd list A, two behind
            // an even one): the staging below moves two entries per lane and round -- one 16-byte key load, one 16-byte LDS write -- and no
            // pair of entries straddles the two lists.  An unusable pair stages nothing (Tb = 0).
            const int mAe = valid ? (mA + 2) & ~1 : 0, Tb = mAe + mB;  // <= TILE + 2: list B's sentinel sB[mB] is entry Tb, the buffers hold TILE + 4
            uint64_t* sB = sA + mAe;
            uint8_t* cB = cA + mAe;

            // lane tl of a team owns merged events [d0, d1) of its pair
            const int epl = (T + TL - 1) / TL;  // <= EPL
            int epl_w = __builtin_amdgcn_readlane(epl, 0);  // wave-uniform trip count: the longest of the teams' chunks
#pragma unroll
            for (int k = 1; k < TEAMS; ++k) epl_w = max(epl_w, __builtin_amdgcn_readlane(epl, k * TL));

            wave_sync_lds();  // the previous pairs' tiles are fully consumed
            {   // stage [A's points | sentinel, pad | B's points]: entries 2 q and 2 q + 1 of the buffer by lane q % TL in round q / TL; all
                // loads before the first LDS write.  The pair of entries behind list A's last point reads one or two store entries past that
                // point, the one that holds list B's last point at most one (still inside the environment's slot or, for the last slot, the
                // bytes the host's arenas leave behind their last array): they land in the sentinel and pad entries, which are rewritten
                // below or never read.
                constexpr int EPL2 = (EPL + 1) / 2;
                static_assert(2 * TL * EPL2 >= TILE_ + 2, "the rounds cover the buffer's used part: TILE points, list A's sentinel and pad entries");
                typedef unsigned long long __attribute__((ext_vector_type(2), aligned(8))) key2_t;
                const int epl2 = (Tb + 2 * TL - 1) / (2 * TL);
                int epl2_w = __builtin_amdgcn_readlane(epl2, 0);
#pragma unroll
                for (int k = 1; k < TEAMS; ++k) epl2_w = max(epl2_w, __builtin_amdgcn_readlane(epl2, k * TL));
                key2_t rk[EPL2];
                uint32_t rc[EPL2];
                // Per-lane state, once per tile: the lane's entry of round 0 in either list, as pointers -- round u lies 2 TL u entries
                // further, a CONSTANT that the loads and the LDS writes carry as their immediate offsets.  A lane crosses from list A to
                // list B once (at the first round with 2 TL u >= toB: mAe and the lane's entry are both even, so no pair straddles): the
                // round picks one of the two pointers.  Rounds with 2 TL u >= left lie behind the buffer's used part: nothing is loaded or
                // written (an unusable pair has Tb = 0: no round at all, its pointers are never followed).
                const int e0 = 2 * tl, toB = mAe - e0, left = Tb - e0;
                const uint64_t* pkA = kA + 1 + e0;
                const uint64_t* pkB = kB + 1 + e0 - mAe;
                const uint8_t* pcA = tA + 1 + e0;
                const uint8_t* pcB = tB + 1 + e0 - mAe;
#pragma unroll
                for (int u = 0; u < EPL2; ++u) { rk[u] = key2_t{0ull, 0ull}; rc[u] = 0u; }
#pragma unroll
                for (int u = 0; u < EPL2; ++u) {
                    if (u < epl2_w) {  // (wave-uniform: rounds no team of this wavefront needs are skipped)
                        if (2 * TL * u < left) {
                            const bool inB = 2 * TL * u >= toB;
                            const uint64_t* src = (inB ? pkB : pkA) + 2 * TL * u;
                            const uint8_t* csrc = (inB ? pcB : pcA) + 2 * TL * u;
                            rk[u] = *reinterpret_cast<const key2_t*>(src);
                            rc[u] = (uint32_t)csrc[0] | ((uint32_t)csrc[1] << 8);
                        }
                    }
                }
                uint64_t* dk = sA + e0;
                uint8_t* dc = cA + e0;
#pragma unroll
                for (int u = 0; u < EPL2; ++u) {
                    if (u < epl2_w) {
                        if (2 * TL * u < left) {
                            *reinterpret_cast<ulonglong2*>(dk + 2 * TL * u) = ulonglong2{rk[u].x, rk[u].y};
                            *reinterpret_cast<uint16_t*>(dc + 2 * TL * u) = (uint16_t)rc[u];
                        }
                    }
                }
                // the two sentinels: larger than every key (the bits of a non-negative finite F), so TeamTile's merge needs no test for
                // the lists' ends.  After the rounds' writes: the staging may have put the store's next entry there, and LDS serves a
                // wavefront's writes in order.
                if (tl == 0 && valid) {
                    sA[mA] = ~0ull;
                    sB[mB] = ~0ull;
                }
            }
            wave_sync_lds();

            // (PRE: the prefix-count rows of the two environments; an unusable pair's records may name slots that do not exist: row 0 of slot 0)
            const uint64_t* preA = PRE ? args.env_a.pre + (valid ? offA / kPreStep * (uint64_t)TT::NW : 0ull) : nullptr;  // (slot strides are multiples of kPreStep)
            const uint64_t* preB = PRE ? args.env_b.pre + (valid ? offB / kPreStep * (uint64_t)TT::NW : 0ull) : nullptr;
            const double acc = TT::run(sA, cA, sB, cB, mA, mB, T, epl, epl_w, c0a, c0b, F0, Finf0, t_sqrt, t_rsqrt, w_s, lcl, tl, preA, preB);
            if (tl == TL - 1 && live && mine) args.out[p] = valid ? acc : nan("");  // (categories were checked when the environments were built)
        }
    }
}

template <int CM, int TM, bool PRE>
static void launch_team_c(hipStream_t s, bool tile240, unsigned grid, int batch, const SweepArgs& a) {
    constexpr int NTH = 64 * kSweepWaves;
    constexpr bool WGT = TM == 1, KSM = TM == 2;
    if (tile240) k_sweep_duo<CM, kDuoTL, kDuoTile, WGT, KSM, PRE><<<grid, NTH, 0, s>>>(a, batch);
    else k_sweep_duo<CM, 32, kTeam8Tile, WGT, KSM, PRE><<<grid, NTH, 0, s>>>(a, batch);
}
template <int TM>
static void launch_team_t(hipStream_t s, int cmax, bool tile240, bool pre, unsigned grid, int batch, const SweepArgs& a) {
    with_slots<kSweepSlots>(cmax, [&](auto S) {
        constexpr int CM = (TM != 0 && S > 16) ? 16 : S;  // (weights / Kolmogorov-Smirnov: at most 16 slots, checked by plan_sweep)
        // both stores carry prefix-count rows of the width this slot count reads (k_env_group wrote them): the PRE instantiations
        if constexpr (TM != 1 && CM <= 16) {
            if (pre && cmax <= 16) return launch_team_c<CM, TM, true>(s, tile240, grid, batch, a);
        }
        launch_team_c<CM, TM, false>(s, tile240, grid, batch, a);
    });
}
void launch_team(hipStream_t s, int cmax, int tm, bool tile240, bool pre, unsigned grid, int batch, const SweepArgs& a) {
    if (tm == 2) launch_team_t<2>(s, cmax, tile240, pre, grid, batch, a);
    else if (tm == 1) launch_team_t<1>(s, cmax, tile240, pre, grid, batch, a);
    else launch_team_t<0>(s, cmax, tile240, pre, grid, batch, a);
}

}  // namespace lchd
