// pg_clip_tubes: every (path, obstacle set) pair of a path library and a library of obstacle sets as a trajectory whose tube is narrowed around the set's discs, on the
// device.  The reference has no obstacles (trajectories.jl:8-44 only stores edge_L, edge_R), so the scheme is build-defined: stated in include/pigeon_mpc.h at
// pg_clip_tubes and in DESIGN.md 4.22, tests/tube_clip_numpy.py is the independent numpy twin.  Included by pg_kernels.hip inside namespace pg.
//
// One workgroup of 256 threads per output trajectory (path * n_sets + set), one launch, knots strided over the threads (thread t owns the knots t, t + 256, ...), phases
// separated by workgroup barriers:  sincos(psi) of a knot, once, into the call's scratch with the two running edges;  per obstacle of the set, in order, the (q, index)
// argmin and the lowest / highest seeing knot by shuffles inside a wavefront and the four wavefront results through LDS, the side decision and the report record by thread 0,
// the side broadcast through LDS, then the hard clip of a thread's own knots;  the taper, (s_k, cL_k, cR_k) staged through LDS in tiles of 256 -- an unclipped knot staged
// as +Inf / -Inf, which no min / max takes, and a tile without a clipped knot skipped --, every thread evaluating every k of a tile for its own knots;  the store and the
// stats.  A thread reads back from the scratch only what it wrote itself.  The source is read as the doubles given, ALL arithmetic is double in both libraries, without
// contraction, and rounded to `real` on store (tools/check_f32_purity.py lists k_tube_clip for this reason, as k_path_offset).  No atomics, no kernel waits on another.

struct ClipSight { double a, b, q, h; int sees; };      // the obstacle in a knot's frame: a to the left, b ahead, q the squared distance, h the half chord on the normal line (0: none)
// Sight of the header: one function for host and device
__host__ __device__ inline ClipSight tc_sight(double E, double N, double sn, double cs, double eL, double eR, double oE, double oN, double R) {
#pragma clang fp contract(off)
    ClipSight S;
    const double wE = oE - E, wN = oN - N;
    const double ncs = -cs, nsn = -sn;
    const double a0 = wE * ncs, a1 = wN * nsn;
    S.a = a0 + a1;
    const double b0 = wE * nsn, b1 = wN * cs;
    S.b = b0 + b1;
    const double q0 = wE * wE, q1 = wN * wN;
    S.q = q0 + q1;
    S.h = 0.0; S.sees = 0;
    if (fabs(S.b) < R) {
        const double rr = R * R, bb = S.b * S.b;
        const double d = rr - bb;
        S.h = sqrt(d);
        const double lo = S.a - S.h, hi = S.a + S.h;
        S.sees = (lo < eL) && (hi > eR);
    }
    return S;
}
// Side of the header at the closest knot: +1 the left edge is clipped, -1 the right one
__host__ __device__ inline int tc_side(int policy, double a_at, double free_left, double free_right) {
    const int centre = a_at > 0.0 ? 1 : -1;
    if (policy == PG_PASS_LEFT) return -1;
    if (policy == PG_PASS_RIGHT) return 1;
    if (policy == PG_PASS_WIDER) { if (free_right > free_left) return 1; if (free_left > free_right) return -1; }
    return centre;
}

// in [n_path][10][Lmax] doubles as the caller gave them; out [n_path * n_sets][10][Lmax]; scratch [6][n_path * n_sets][Lmax] doubles: sin psi, cos psi, cL, cR and the two
// tapered edges of a knot; report [n_path * n_sets][max_count]
struct TubeClipArgs { int n_sets, Lmax, max_count; const int* L; const int* closed; const double* in; const pg_obstacle_set* sets; const pg_obstacle* obs; real* out; double* scratch;
                      double* t_end; pg_clip_stats* stats; pg_obstacle_report* report; };
enum { TC_THREADS = 256, TC_WAVES = TC_THREADS / 64 };

__global__ __launch_bounds__(TC_THREADS) void k_tube_clip(TubeClipArgs P) {
#pragma clang fp contract(off)
    __shared__ double sQ[TC_WAVES];                               // the smallest q (then: the smallest width) of a wavefront
    __shared__ int sK[TC_WAVES][3];                               // its knot, the lowest and the highest seeing knot
    __shared__ int sSide;
    __shared__ double sS[TC_THREADS], sL[TC_THREADS], sR[TC_THREADS];      // a tile of the taper: s_k, cL_k or +Inf, cR_k or -Inf
    __shared__ int sAny;
    __shared__ int sN[TC_WAVES][4];                               // n_clip_L, n_clip_R, n_blocked, n_centre_out
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t k = blockIdx.x, Lmax = (size_t)P.Lmax, n_traj = (size_t)gridDim.x;
    const int path = (int)(k / (size_t)P.n_sets), set = (int)(k - (size_t)path * P.n_sets);
    const pg_obstacle_set S = P.sets[set];
    const int n = P.L[path];
    const bool closed = P.closed[path] != 0;
    const int nk = closed ? n - 1 : n;                            // the knots that take part: knot L-1 of a closed path is knot 0 again
    const double* __restrict__ src = P.in + (size_t)path * 10 * Lmax;      // every knot index below is < n <= Lmax
    const double* __restrict__ s = src + PO_S * Lmax; const double* __restrict__ E = src + PO_E * Lmax; const double* __restrict__ N = src + PO_N * Lmax;
    const double* __restrict__ eL = src + PO_EL * Lmax; const double* __restrict__ eR = src + PO_ER * Lmax;
    real* const o = P.out + k * 10 * Lmax;
    const size_t plane = n_traj * Lmax;
    double* const sn = P.scratch + k * Lmax; double* const cs = sn + plane; double* const cL = cs + plane; double* const cR = cL + plane;
    double* const tL = cR + plane; double* const tR = tL + plane;
    pg_obstacle_report* const rep = P.report + k * (size_t)P.max_count;

    // ---- sincos(psi) of a knot, once; the running edges start from the source's ----
    for (int i = tid; i < nk; i += TC_THREADS) {
        double a, b;
        sincos(src[PO_PSI * Lmax + i], &a, &b);
        sn[i] = a; cs[i] = b; cL[i] = eL[i]; cR[i] = eR[i];
    }
    // ---- the obstacles of the set, in order ----
    int n_seen = 0, n_ignored = 0;
    for (int j = 0; j < S.count; j++) {
        const pg_obstacle O = P.obs[S.first + j];
        const double R = O.radius + S.margin;
        double qb = INFINITY; int kb = 0x7fffffff, kf = 0x7fffffff, kl = -1;
        for (int i = tid; i < nk; i += TC_THREADS) {
            const ClipSight G = tc_sight(E[i], N[i], sn[i], cs[i], eL[i], eR[i], O.E, O.N, R);
            if (G.q < qb || kb == 0x7fffffff) { qb = G.q; kb = i; }      // (ascending i: the lowest index on ties; a thread's first knot whatever its q, so kb is a knot)
            if (G.sees) { kf = min(kf, i); kl = i; }
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const double q2 = __shfl_xor(qb, d, 64); const int k2 = __shfl_xor(kb, d, 64);
            if (q2 < qb || (q2 == qb && k2 < kb)) { qb = q2; kb = k2; }
            kf = min(kf, __shfl_xor(kf, d, 64)); kl = max(kl, __shfl_xor(kl, d, 64));
        }
        if (lane == 0) { sQ[wave] = qb; sK[wave][0] = kb; sK[wave][1] = kf; sK[wave][2] = kl; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < TC_WAVES; w++) {
                if (sQ[w] < qb || (sQ[w] == qb && sK[w][0] < kb)) { qb = sQ[w]; kb = sK[w][0]; }
                kf = min(kf, sK[w][1]); kl = max(kl, sK[w][2]);
            }
            const ClipSight G = tc_sight(E[kb], N[kb], sn[kb], cs[kb], eL[kb], eR[kb], O.E, O.N, R);      // (sn, cs of another thread's knot: written before the barrier above)
            pg_obstacle_report r;
            r.u_at = s[kb] - s[0]; r.a_at = G.a; r.h_at = G.h; r.dist_at = sqrt(G.q);
            const double lo = G.a - G.h, hi = G.a + G.h;
            r.free_right = lo - eR[kb]; r.free_left = eL[kb] - hi;
            r.k_at = kb;
            const bool seen = kl >= 0;
            r.k_first = seen ? kf : -1; r.k_last = seen ? kl : -1;
            r.side = seen ? tc_side(S.policy, G.a, r.free_left, r.free_right) : 0;
            rep[j] = r;
            sSide = r.side;
            n_seen += seen; n_ignored += !seen;
        }
        __syncthreads();
        const int side = sSide;
        if (side != 0) {
            for (int i = tid; i < nk; i += TC_THREADS) {
                const ClipSight G = tc_sight(E[i], N[i], sn[i], cs[i], eL[i], eR[i], O.E, O.N, R);
                if (!G.sees) continue;
                if (side > 0) cL[i] = fmin(cL[i], G.a - G.h); else cR[i] = fmax(cR[i], G.a + G.h);
            }
        }
    }
    // the unused slots of the report: all zero, the knots -1
    for (int j = S.count + tid; j < P.max_count; j += TC_THREADS) {
        pg_obstacle_report r;
        r.u_at = 0.0; r.a_at = 0.0; r.h_at = 0.0; r.dist_at = 0.0; r.free_left = 0.0; r.free_right = 0.0; r.k_at = -1; r.k_first = -1; r.k_last = -1; r.side = 0;
        rep[j] = r;
    }
    // ---- the taper ----
    for (int i = tid; i < nk; i += TC_THREADS) { tL[i] = cL[i]; tR[i] = cR[i]; }
    if (S.taper < INFINITY) {
        const double m = S.taper, per = s[n - 1] - s[0];
        for (int base = 0; base < nk; base += TC_THREADS) {
            __syncthreads();                                      // (the tile before has been read; the first time round: sAny is free)
            if (tid == 0) sAny = 0;
            __syncthreads();
            const int kk = base + tid;
            double a = 0.0, l = INFINITY, r = -INFINITY;
            if (kk < nk) {
                a = s[kk];
                if (cL[kk] < eL[kk]) l = cL[kk];
                if (cR[kk] > eR[kk]) r = cR[kk];
            }
            sS[tid] = a; sL[tid] = l; sR[tid] = r;
            if (l < INFINITY || r > -INFINITY) sAny = 1;          // (every writer stores the same value)
            __syncthreads();
            if (!sAny) continue;                                  // no clipped knot in the tile: every term is +Inf / -Inf
            const int cnt = min(TC_THREADS, nk - base);
            for (int i = tid; i < nk; i += TC_THREADS) {
                const double si = s[i];
                double vl = tL[i], vr = tR[i];
                for (int c = 0; c < cnt; c++) {
                    const double diff = si - sS[c];
                    double dist = fabs(diff);
                    if (closed) { const double alt = per - dist; dist = fmin(dist, alt); }
                    const double md = m * dist;
                    vl = fmin(vl, sL[c] + md); vr = fmax(vr, sR[c] - md);
                }
                tL[i] = vl; tR[i] = vr;
            }
        }
    }
    // ---- the store and the stats ----
    int ncl = 0, ncr = 0, nbl = 0, nco = 0;
    double wb = INFINITY; int kw = 0x7fffffff;
    for (int i = tid; i < n; i += TC_THREADS) {
        for (int ch = 0; ch < PO_EL; ch++) o[ch * Lmax + i] = (real)src[ch * Lmax + i];
        if (i >= nk) continue;                                    // knot L-1 of a closed path: its edges are knot 0's, below
        const double l = tL[i], r = tR[i];
        o[PO_EL * Lmax + i] = (real)l; o[PO_ER * Lmax + i] = (real)r;
        if (closed && i == 0) { o[PO_EL * Lmax + nk] = (real)l; o[PO_ER * Lmax + nk] = (real)r; }
        const double w = l - r;
        ncl += l != eL[i]; ncr += r != eR[i]; nbl += w < S.min_width; nco += !(r < 0.0 && 0.0 < l);
        if (w < wb || kw == 0x7fffffff) { wb = w; kw = i; }
    }
    // every channel is 0 at and past L
    const size_t tail = Lmax - (size_t)n;
    for (size_t e = tid; e < 10 * tail; e += TC_THREADS) { const size_t ch = e / tail; o[ch * Lmax + (size_t)n + (e - ch * tail)] = real(0.0); }
    for (int d = 32; d >= 1; d >>= 1) {
        const double w2 = __shfl_xor(wb, d, 64); const int k2 = __shfl_xor(kw, d, 64);
        if (w2 < wb || (w2 == wb && k2 < kw)) { wb = w2; kw = k2; }
        ncl += __shfl_xor(ncl, d, 64); ncr += __shfl_xor(ncr, d, 64); nbl += __shfl_xor(nbl, d, 64); nco += __shfl_xor(nco, d, 64);
    }
    __syncthreads();                                              // (sQ, sK of the last obstacle have been read)
    if (lane == 0) { sQ[wave] = wb; sK[wave][0] = kw; sN[wave][0] = ncl; sN[wave][1] = ncr; sN[wave][2] = nbl; sN[wave][3] = nco; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < TC_WAVES; w++) {
            if (sQ[w] < wb || (sQ[w] == wb && sK[w][0] < kw)) { wb = sQ[w]; kw = sK[w][0]; }
            ncl += sN[w][0]; ncr += sN[w][1]; nbl += sN[w][2]; nco += sN[w][3];
        }
        pg_clip_stats T;
        T.width_min = wb; T.u_width_min = s[kw] - s[0]; T.reserved_d[0] = 0.0; T.reserved_d[1] = 0.0;
        T.n_clip_L = ncl; T.n_clip_R = ncr; T.n_blocked = nbl; T.n_centre_out = nco; T.n_seen = n_seen; T.n_ignored = n_ignored; T.reserved[0] = 0; T.reserved[1] = 0;
        P.stats[k] = T;
        P.t_end[k] = (double)(real)src[PO_T * Lmax + (n - 1)];      // trajectory.t[end] as the library holds it
    }
}
