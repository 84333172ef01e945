// Snapshot / restore of the episode state (gfx950 / CDNA4, wave64): the gather-copy kernels behind vds_snapshot / vds_restore /
// vds_restore_device (vds.h).  One body per table shape serves both directions:
//   snapshot   live tables -> store, identity map (map == nullptr)
//   restore    store -> live tables, replica r continues from the store's replica map[r] (stored replica indices)
// Source and destination are always different allocations with the same strides, so nothing is copied in place.  The work is a pure
// copy and the only roof is HBM: every variable-length row is copied up to its clamped LIVE length, read from the SOURCE side's own
// counts (the source's bucket records / ring counts - never from a table another launch of the same call writes).
// Three shapes:
//   1. k_snap_rows    short rows with a per-row length: idle, ring, ring_min, fl, inbox - tables [A][R][cap] (A = C, H * C, 2 * C).
//                     SN_LPR lanes per row, the rows of a wavefront are consecutive replicas of one plane a (the count loads and the
//                     map loads of a wavefront are one or two contiguous segments); data moves in 16-byte pieces - every capacity is
//                     a multiple of 16 entries, so a length rounded up to a piece stays inside its row; a group keeps SN_RPT rows in
//                     flight, because each row is a dependent chain count -> data (k_idle_heads, IH_RPT).  One body for the 4-, 8-
//                     and 16-byte entries of the dense and the wide layout: the entry size is a parameter.
//   2. k_snap_gather  fixed records and words gathered along R: hdr, cnt (64-byte records), ring_cnt, sup, arr (words) - tables
//                     [A][R]: dst[a][r] = src[a][map[r]], lanes along r, SN_GA planes a per thread behind one map load.
//   3. k_snap_out     long rows: out [R][Oq], the prefix of orders processed so far on the replica's day; workgroup chunks of a
//                     row in 16-byte pieces (8-byte pieces when Oq is odd: rows are then only 8-byte aligned).
// k_snap_prep turns a caller's device-resident map into the handle-owned one the copies read: an entry outside [0, R) leaves that
// replica on its own row and raises ERR_RESTORE; it also sets the supply planes' slot word to the restored slot's.
// Plain vector loads and stores; no LDS, no inline assembly; the only atomic is the error bit.
// The lists are compact at every API boundary (HDR_RAW == 0: vds_step and vds_run_hooked flush the stamp form every slot, vds_run
// behind its last slot) and every stamp is 0xFFFF then - the stamp table needs no copy; HDR_RAW is checked in the WKDEBUG build.
// This file is hashed with the HOST sources (Makefile): it is not one of the tick kernels the profiles/ evidence refers to.
#include "vds_kernels_common.h"
#include "vds_launch.h"
#ifdef WKDEBUG
#include <cstdio>
#endif

namespace vds {

#define SN_THREADS 256
#define SN_LPR 8                 // lanes per row (k_snap_rows): 8 x 16 B = 128 B per step
#define SN_RPT 4                 // rows per lane group, their loads in flight together
#define SN_GA 4                  // planes per thread (k_snap_gather)
#define SN_OPT 4                 // pieces per thread (k_snap_out)

// where k_snap_rows finds the length of row (a, r): cnt[((a % mod) * R + r) * stride + word + a / mod] & mask
//   idle   hdr, stride HDR_WORDS, mod C, word HDR_IDLE              ring / ring_min   ring_cnt, stride 1, mod H * C, word 0, low 16 bits
//   fl     hdr, ...,               word HDR_FL                      inbox (2 parities) hdr, mod C, word HDR_INBOX0 (+ parity = a / C)
struct SnapLen { const int *cnt; int stride, mod, word, mask; };

// src / dst: [A][R][cap] entries of `es` bytes (cap * es a multiple of 16).  Grid: x = (runs of SN_THREADS / SN_LPR * SN_RPT replicas) x A.
__global__ __launch_bounds__(SN_THREADS) void k_snap_rows(const uint4 *__restrict__ src, uint4 *__restrict__ dst, SnapLen L, const int *__restrict__ map,
                                                         int R, int A, int cap, int es, int rblocks) {
    const int a = (int)(blockIdx.x / (unsigned)rblocks), rb = (int)(blockIdx.x % (unsigned)rblocks);
    if (a >= A) return;
    const int g = (int)threadIdx.x / SN_LPR, lg = (int)threadIdx.x % SN_LPR;
    const int GROUPS = SN_THREADS / SN_LPR;
    const int row16 = (cap * es) >> 4;                         // 16-byte pieces of a whole row
    const int ca = a % L.mod, cw = L.word + a / L.mod;
    int sr[SN_RPT], r[SN_RPT];
#pragma unroll
    for (int u = 0; u < SN_RPT; ++u) {
        r[u] = rb * (GROUPS * SN_RPT) + u * GROUPS + g;
        sr[u] = r[u] < R ? (map ? map[r[u]] : r[u]) : -1;
    }
    int np[SN_RPT], maxp = 0;
#pragma unroll
    for (int u = 0; u < SN_RPT; ++u) {
        np[u] = 0;
        if (sr[u] < 0) continue;
        const int *cp = L.cnt + ((size_t)ca * R + sr[u]) * L.stride;
        const int n = min(max(cp[cw] & L.mask, 0), cap);      // (an overflowed ring slot counts beyond its capacity)
#ifdef WKDEBUG
        if (L.stride == HDR_WORDS && L.word == HDR_IDLE && lg == 0 && cp[HDR_RAW] != 0) printf("k_snap_rows: raw list (HDR_RAW %d) c %d r %d\n", cp[HDR_RAW], ca, sr[u]);
#endif
        np[u] = min((n * es + 15) >> 4, row16);
        maxp = max(maxp, np[u]);
    }
    for (int p = lg; p < maxp; p += SN_LPR) {
        uint4 v[SN_RPT];
#pragma unroll
        for (int u = 0; u < SN_RPT; ++u) {
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            if (p < np[u]) v[u] = src[((size_t)a * R + sr[u]) * row16 + p];
        }
#pragma unroll
        for (int u = 0; u < SN_RPT; ++u)
            if (p < np[u]) dst[((size_t)a * R + r[u]) * row16 + p] = v[u];
    }
}

// src / dst: [A][R] records of `per` elements T (per = 1: words; per = 4, T = uint4: 64-byte records).  Thread i of a replica run owns
// element i % per of replica i / per and walks SN_GA planes.  Grid: x = (runs of SN_THREADS / per replicas) x (runs of SN_GA planes).
template <typename T>
__global__ __launch_bounds__(SN_THREADS) void k_snap_gather(const T *__restrict__ src, T *__restrict__ dst, const int *__restrict__ map, int R, long long A, int per, int rblocks) {
    const long long a0 = (long long)(blockIdx.x / (unsigned)rblocks) * SN_GA;
    const int i = (int)(blockIdx.x % (unsigned)rblocks) * SN_THREADS + (int)threadIdx.x;
    const int r = i / per, e = i - r * per;
    if (r >= R) return;
    const int sr = map ? map[r] : r;
    T v[SN_GA];
#pragma unroll
    for (int u = 0; u < SN_GA; ++u) {
        v[u] = T{};
        if (a0 + u < A) v[u] = src[((size_t)(a0 + u) * R + sr) * per + e];
    }
#pragma unroll
    for (int u = 0; u < SN_GA; ++u)
        if (a0 + u < A) dst[((size_t)(a0 + u) * R + r) * per + e] = v[u];
}

// out [R][Oq] {veh, wait}: row r <- row map[r], the results of the orders of slots [0, tdone) of the replica's day (bkt_off of its
// day through day_view; a day that is over: all of it).  P: uint4 (Oq even) or uint2.  Grid: x = replica x (chunks of SN_THREADS * SN_OPT pieces).
template <typename P>
__global__ __launch_bounds__(SN_THREADS) void k_snap_out(Static S, const int2 *__restrict__ src, int2 *__restrict__ dst, const int *__restrict__ map, int tdone, int chunks) {
    const int r = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
    const int sr = map ? map[r] : r;
    const DayView dv = day_view(S, sr);
    const int n = min(max(dv.bkt_off[(size_t)min(tdone, dv.T) * S.C] - dv.q_base, 0), S.Oq);      // processed orders: the row's live prefix
    const int EPP = (int)(sizeof(P) / sizeof(int2));
    const int np = (n + EPP - 1) / EPP;
    const int p0 = chunk * (SN_THREADS * SN_OPT) + (int)threadIdx.x;
    if (chunk * (SN_THREADS * SN_OPT) >= np) return;
    const P *s = reinterpret_cast<const P *>(src + (size_t)sr * S.Oq);
    P *d = reinterpret_cast<P *>(dst + (size_t)r * S.Oq);
    P v[SN_OPT];
#pragma unroll
    for (int u = 0; u < SN_OPT; ++u) {
        v[u] = P{};
        if (p0 + u * SN_THREADS < np) v[u] = s[p0 + u * SN_THREADS];
    }
#pragma unroll
    for (int u = 0; u < SN_OPT; ++u)
        if (p0 + u * SN_THREADS < np) d[p0 + u * SN_THREADS] = v[u];
}

// user: the caller's device map [R] (null: `map` was uploaded by the host, checked there).  sup_slot (nullable): the supply planes' slot word.
__global__ __launch_bounds__(SN_THREADS) void k_snap_prep(const int *__restrict__ user, int *__restrict__ map, int R, int *err, int *sup_slot, int sup_val) {
    const int r = (int)blockIdx.x * SN_THREADS + (int)threadIdx.x;
    if (r == 0 && sup_slot != nullptr) sup_slot[0] = sup_val;
    if (r >= R || user == nullptr) return;
    int m = user[r];
    if (m < 0 || m >= R) { m = r; atomicOr(&err[0], ERR_RESTORE); }
    map[r] = m;
}

void emit_snap_prep(const Emit &e, const int *user, int *map, int R, int *err, int *sup_slot, int sup_val) {
    emit_kernel(e, k_snap_prep, dim3((R + SN_THREADS - 1) / SN_THREADS), dim3(SN_THREADS), 0, user, map, R, err, sup_slot, sup_val);
}

static void emit_rows(const Emit &e, const void *src, void *dst, SnapLen L, const int *map, int R, long long A, int cap, int es) {
    if (!src || !dst || A <= 0 || R <= 0) return;
    const int per_block = SN_THREADS / SN_LPR * SN_RPT;
    const int rblocks = (R + per_block - 1) / per_block;
    emit_kernel(e, k_snap_rows, dim3((unsigned)(A * rblocks)), dim3(SN_THREADS), 0, reinterpret_cast<const uint4 *>(src), reinterpret_cast<uint4 *>(dst), L, map, R, (int)A, cap, es, rblocks);
}
template <typename T>
static void emit_gather(const Emit &e, const void *src, void *dst, const int *map, int R, long long A, int per) {
    if (!src || !dst || A <= 0 || R <= 0) return;
    const int rblocks = (int)(((long long)R * per + SN_THREADS - 1) / SN_THREADS);
    const long long ablocks = (A + SN_GA - 1) / SN_GA;
    emit_kernel(e, k_snap_gather<T>, dim3((unsigned)(ablocks * rblocks)), dim3(SN_THREADS), 0, reinterpret_cast<const T *>(src), reinterpret_cast<T *>(dst), map, R, A, per, rblocks);
}

// One table of the snapshot (SNAP_* of vds_launch.h) from `src` to `dst` (State views of the live tables / of the store).  A table the
// layout does not have (null on either side) launches nothing.  tdone: slots whose orders have been processed (SNAP_OUT only).
void emit_snap_table(const Emit &e, const Static &S, const State &src, const State &dst, const int *map, int table, int tdone) {
    const int R = S.R, C = S.C;
    const long long HC = (long long)S.H * C;
    const SnapLen by_hdr{src.hdr, HDR_WORDS, C, 0, 0x7FFFFFFF}, by_ring{src.ring_cnt, 1, (int)HC, 0, 0xFFFF};
    SnapLen L = by_hdr;
    switch (table) {
    case SNAP_IDLE:     L.word = HDR_IDLE;   emit_rows(e, src.idle, dst.idle, L, map, R, C, S.idle_cap, S.dense ? 4 : 8); break;
    case SNAP_RING:     emit_rows(e, src.ring, dst.ring, by_ring, map, R, HC, S.ring_cap, S.dense ? 8 : 16); break;
    case SNAP_RING_MIN: emit_rows(e, src.ring_min, dst.ring_min, by_ring, map, R, HC, S.ring_cap, 4); break;
    case SNAP_FL:       L.word = HDR_FL;     emit_rows(e, src.fl, dst.fl, L, map, R, C, S.fl_cap, 16); break;
    case SNAP_INBOX:    L.word = HDR_INBOX0; emit_rows(e, src.inbox, dst.inbox, L, map, R, 2 * (long long)C, S.in_cap, 16); break;
    case SNAP_HDR:      emit_gather<uint4>(e, src.hdr, dst.hdr, map, R, C, HDR_WORDS * 4 / 16); break;
    case SNAP_CNT:      emit_gather<uint4>(e, src.cnt, dst.cnt, map, R, C, CNT_WORDS * 8 / 16); break;
    case SNAP_RING_CNT: emit_gather<unsigned>(e, src.ring_cnt, dst.ring_cnt, map, R, HC, 1); break;
    case SNAP_SUP:      emit_gather<unsigned>(e, src.sup, dst.sup, map, R, (long long)VDS_SUP_PLANES * C, 1); break;
    case SNAP_ARR:      emit_gather<unsigned>(e, src.arr, dst.arr, map, R, S.pull ? S.arr_slots : 0, 1); break;
    case SNAP_OUT: {
        if (!src.out || !dst.out || S.Oq <= 0 || R <= 0) break;
        const int epp = S.Oq % 2 == 0 ? 2 : 1;
        const int chunks = ((S.Oq + epp - 1) / epp + SN_THREADS * SN_OPT - 1) / (SN_THREADS * SN_OPT);
        const dim3 grid((unsigned)((long long)chunks * R)), block(SN_THREADS);
        if (epp == 2) emit_kernel(e, k_snap_out<uint4>, grid, block, 0, S, src.out, dst.out, map, tdone, chunks);
        else emit_kernel(e, k_snap_out<uint2>, grid, block, 0, S, src.out, dst.out, map, tdone, chunks);
        break;
    }
    default: break;
    }
}

}  // namespace vds
