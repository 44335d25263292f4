// pg_hji_solve: the backward reachable tube of the 7-D relative system on the device -- the computation behind the reference's downloaded deps/BicycleCAvoid.jld2
// (deps/build.jl:1-4; an external level-set toolbox made that file, the reference holds no solver).  Build-defined numerics, stated in include/pigeon_mpc.h at
// pg_hji_solve and in DESIGN.md; tests/hji_solve_numpy.py is the independent numpy twin.  Included by pg_kernels.hip inside namespace pg, after the device functions
// it reuses: hji_optimal_control (:133-158, uMode = :max, N = 50), optimal_disturbance (:90-131, dMode = :min) and world_body_rhs (relative_dynamics :74-88).
//
// One sweep = two launches, thread = node, dimension 1 along the lanes (the loads of V at +-e_d, d >= 2, are as coalesced as the loads of V itself):
//   k_hji_sweep_eval    p-, p+ from the 14-point stencil -> pbar -> uR*, uH* -> f = relative_dynamics -> Hc[node] = pbar . f;  alpha_d = max |f_d| (wave shuffles, the block's
//                       four waves through LDS, ONE atomic max per block and dimension on the bit pattern of the non-negative number: order-independent, so reproducible)
//   k_hji_sweep_update  the stencil again (a re-read of V, not of the 50-point line search) -> Hhat = Hc + sum_d alpha_d (p+_d - p-_d) / 2 -> Vn = float32(V + dt min(0, Hhat))
// dt is formed on the host from alpha between the two launches (the only loop over sweeps is the host's).  V is ping-ponged: no kernel reads what it writes.
// k_hji_finish writes the node records (V, gradV = pbar of the final V) pg_set_hji_grid uploads -- the install path takes them from there -- and reduces min / max V.
//
// The stencil reads V straight from global memory: the eval pass is bound by the line search (200 Fiala evaluations a node), not by its 15 loads of V, which the L2 serves
// (measured); an LDS plane of dimensions 1 x 2 would save loads the pass does not wait for.

struct HjiSolveGrid { int dims[7]; int koff[7]; long stride[7]; long n; int periodic; const float* knots; };

PG_DEV void hji_node_index(const HjiSolveGrid& G, long node, int idx[7]) {
    long rem = node;
#pragma unroll
    for (int d = 0; d < 7; d++) { idx[d] = (int)(rem % G.dims[d]); rem /= G.dims[d]; }
}

// one-sided differences of V at `node` over the actual spacings.  A low face takes p- := p+, a high face p+ := p-; with `periodic` dimension 3 wraps (first and last knot
// are the same angle): the low neighbour of node 0 is node n-2 at spacing x[n-1] - x[n-2], the high neighbour of node n-1 is node 1 at spacing x[1] - x[0].
// Every neighbour index lies in [0, dims[d]): no load leaves the array.
PG_DEV void hji_stencil(const HjiSolveGrid& G, const float* __restrict__ V, long node, const int idx[7], real pm[7], real pp[7]) {
    const real v = (real)V[node];
#pragma unroll
    for (int d = 0; d < 7; d++) {
        const int i = idx[d], n = G.dims[d];
        const float* k = G.knots + G.koff[d];
        const bool wrap = d == 2 && G.periodic;
        bool has_lo = i > 0, has_hi = i < n - 1;
        long nlo = node - G.stride[d], nhi = node + G.stride[d];
        int klo = i, khi = i + 1;                                   // spacing of the low side = k[klo] - k[klo-1], of the high side = k[khi] - k[khi-1]
        if (wrap && !has_lo) { nlo = node + (long)(n - 2) * G.stride[d]; klo = n - 1; has_lo = true; }
        if (wrap && !has_hi) { nhi = node - (long)(n - 2) * G.stride[d]; khi = 1; has_hi = true; }
        real a = real(0.0), b = real(0.0);
        if (has_lo) a = (v - (real)V[nlo]) / ((real)k[klo] - (real)k[klo - 1]);
        if (has_hi) b = ((real)V[nhi] - v) / ((real)k[khi] - (real)k[khi - 1]);
        pm[d] = has_lo ? a : b; pp[d] = has_hi ? b : a;
    }
}

// the state of a node.  Under the periodic flag the last psi node is evaluated at the FIRST knot's angle (the same angle): both copies see the same sine and cosine, so
// they stay bit-identical whenever V does
PG_DEV void hji_node_state(const HjiSolveGrid& G, const int idx[7], real x[7]) {
#pragma unroll
    for (int d = 0; d < 7; d++) {
        int i = idx[d];
        if (d == 2 && G.periodic && i == G.dims[d] - 1) i = 0;
        x[d] = (real)G.knots[G.koff[d] + i];
    }
}

#ifdef PG_F32
PG_DEV void hji_atomic_max_nonneg(real* p, real v) { atomicMax(reinterpret_cast<unsigned int*>(p), __float_as_uint(v)); }
#else
PG_DEV void hji_atomic_max_nonneg(real* p, real v) { atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v)); }
#endif

__global__ __launch_bounds__(256) void k_hji_sweep_eval(HjiSolveGrid G, DevVehicle P, const float* __restrict__ V, real* __restrict__ Hc, real* __restrict__ alpha) {
    const long node = (long)blockIdx.x * 256 + threadIdx.x;
    real af[7];
#pragma unroll
    for (int d = 0; d < 7; d++) af[d] = real(0.0);
    if (node < G.n) {
        int idx[7]; real pm[7], pp[7], g[7], x[7];
        hji_node_index(G, node, idx);
        hji_stencil(G, V, node, idx, pm, pp);
        hji_node_state(G, idx, x);
#pragma unroll
        for (int d = 0; d < 7; d++) g[d] = (pp[d] + pm[d]) * real(0.5);
        real d_opt, Fx_opt, w = real(0.0), a = real(0.0);
        hji_optimal_control(P, x, g, d_opt, Fx_opt);
        if (x[5] > real(0.0)) optimal_disturbance(P, x, g, w, a);           // (a stopped car has no worst case: (0, 0), as human_control defines it)
        real dUx, dUy, dr;
        world_body_rhs<real>(P, x[3], x[4], x[6], d_opt, Fx_opt, dUx, dUy, dr);
        real s, c; pg_sincos(x[2], &s, &c);
        real f[7];
        f[0] = x[5] * c - x[3] + x[1] * x[6]; f[1] = x[5] * s - x[4] - x[0] * x[6]; f[2] = w - x[6]; f[3] = dUx; f[4] = dUy; f[5] = a; f[6] = dr;
        real H = real(0.0);
#pragma unroll
        for (int d = 0; d < 7; d++) { H += g[d] * f[d]; af[d] = fabs(f[d]); }
        Hc[node] = H;
    }
    __shared__ real red[4][7];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 0; d < 7; d++) {
        real v = af[d];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
        if (lane == 0) red[wave][d] = v;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int d = threadIdx.x;
        hji_atomic_max_nonneg(alpha + d, fmax(fmax(red[0][d], red[1][d]), fmax(red[2][d], red[3][d])));
    }
}

__global__ __launch_bounds__(256) void k_hji_sweep_update(HjiSolveGrid G, const float* __restrict__ V, const real* __restrict__ Hc, const real* __restrict__ alpha, real dt,
                                                          float* __restrict__ Vn, int* __restrict__ bad) {
    const long node = (long)blockIdx.x * 256 + threadIdx.x;
    if (node >= G.n) return;
    int idx[7]; real pm[7], pp[7];
    hji_node_index(G, node, idx);
    hji_stencil(G, V, node, idx, pm, pp);
    real diss = real(0.0);
#pragma unroll
    for (int d = 0; d < 7; d++) diss += alpha[d] * (pp[d] - pm[d]) * real(0.5);
    const real Hh = Hc[node] + diss;
    const float o = (float)((real)V[node] + dt * jmin(real(0.0), Hh));      // (jmin: a NaN stays a NaN and is reported, it is not clipped to 0)
    Vn[node] = o;
    if (!(fabsf(o) <= 3.4028234663852886e38f)) atomicOr(bad, 1);
}

// monotone map of a float onto unsigned integers (so that integer atomic min / max order floats of either sign)
PG_DEV unsigned int hji_float_key(float v) { const unsigned int b = __float_as_uint(v); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }

// node records (V, gradV[0..6]) of the final V, 32 B per node as pg_set_hji_grid interleaves them; vkeys[0] / vkeys[1] = min / max of V as hji_float_key
__global__ __launch_bounds__(256) void k_hji_finish(HjiSolveGrid G, const float* __restrict__ V, float* __restrict__ rec, unsigned int* __restrict__ vkeys, int* __restrict__ bad) {
    const long node = (long)blockIdx.x * 256 + threadIdx.x;
    float vlo = INFINITY, vhi = -INFINITY;
    if (node < G.n) {
        int idx[7]; real pm[7], pp[7];
        hji_node_index(G, node, idx);
        hji_stencil(G, V, node, idx, pm, pp);
        const float v = V[node];
        float g[7];
#pragma unroll
        for (int d = 0; d < 7; d++) g[d] = (float)((pp[d] + pm[d]) * real(0.5));
        float4* o = reinterpret_cast<float4*>(rec + node * 8);
        o[0] = make_float4(v, g[0], g[1], g[2]); o[1] = make_float4(g[3], g[4], g[5], g[6]);
        vlo = v; vhi = v;
        if (!(fabsf(v) <= 3.4028234663852886e38f)) atomicOr(bad, 1);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { vlo = fminf(vlo, __shfl_xor(vlo, off, 64)); vhi = fmaxf(vhi, __shfl_xor(vhi, off, 64)); }
    if ((threadIdx.x & 63) == 0 && vlo <= vhi) {
        // (the stored keys only move one way, so a relaxed read skips the atomics that could not win: 156 k wavefronts on two addresses took 3.5 ms without it)
        const unsigned int klo = hji_float_key(vlo), khi = hji_float_key(vhi);
        if (klo < __atomic_load_n(vkeys, __ATOMIC_RELAXED)) atomicMin(vkeys, klo);
        if (khi > __atomic_load_n(vkeys + 1, __ATOMIC_RELAXED)) atomicMax(vkeys + 1, khi);
    }
}
