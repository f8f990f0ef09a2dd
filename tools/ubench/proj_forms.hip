// Micro-benchmark (gfx950): the per-(item, view) projection and normalisation chain of mh_search3_kernel (csrc/mh_device.h:
// mh_pixel_of_fast1 + mh_unit2_fast1) for FOUR items per lane, in three forms --
//   P  two packed pairs: the chain on 64-bit register pairs, v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 (the form the search ran)
//   S  four plain chains, the compiler's schedule
//   G  four plain chains, items 0-1 in front of a scheduling barrier, items 2-3 behind it (divisions and roots pair by pair)
// at 5 waves per SIMD (1280 workgroups of 256 lanes, held to 5 by amdgpu_waves_per_eu): ALONE (every workgroup projects); MIXED
// (every fifth workgroup projects, the other four run the key block of the tap loop -- 4 taps x 4 items: mul, mul, add, sub,
// v_lshl_or, half a v_min3 per evaluation, tools/ubench/valu5.hip N1 -- until the projecting workgroups are done, or a cap);
// and ALTERNATING, the shape of the search kernel itself: every wave projects its four items and then runs 12 key blocks (48 taps) on
// the directions it has just made, 2000 times over, the workgroups starting 0, 2, 4, 7 and 9 blocks into that cycle -- so that a wave which
// projects does so beside waves in their key blocks.  Its cost of a visit is the launch time over the same launch without the projection.
// Prints, per form, the time of one (wave, view) visit as the wave sees it and as the SIMD pays for it (ALONE: the wave's time / 5 waves;
// ALTERNATING: the difference of the launch times / visits / 5 waves), in ns and in cycles at an assumed 2.4 GHz; MIXED: the wave's time
// and the rate of the key blocks beside it.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -o /tmp/proj_forms tools/ubench/proj_forms.hip && /tmp/proj_forms
// (the flags of csrc/pmvo_search.hip's own build line: without -fno-slp-vectorize the compiler packs S and G again)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

#define WGS 1280     // 256 CUs x 5 workgroups: 5 waves on every SIMD
#define SIMDS 1024
#define CAM 24       // floats per camera record of the table (0-11, 16, 18, 21, 22 as in mh_pixel_of_fast1; 12, 13: the patch centre)
typedef float v2 __attribute__((ext_vector_type(2)));
#define DEV __device__ __forceinline__

DEV float fma1(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
DEV v2 fma2(v2 a, v2 b, v2 c) { return __builtin_elementwise_fma(a, b, c); }
DEV v2 splat(float x) { return v2{x, x}; }

DEV float sqrt_before_clamp(float x) {
    float r = __builtin_amdgcn_sqrtf(x);
    const float rd = __uint_as_float(__float_as_uint(r) - 1u), ru = __uint_as_float(__float_as_uint(r) + 1u);
    const float ed = fma1(-rd, r, x), eu = fma1(-ru, r, x);
    r = (0.0f >= ed) ? rd : r;
    r = (0.0f < eu) ? ru : r;
    return r;
}

// ---- one item on plain registers
DEV void div1x2(float n0, float n1, float d, float &q0, float &q1) {
    float r = __builtin_amdgcn_rcpf(d);
    const float nd = -d;
    const float e = fma1(nd, r, 1.0f);
    r = fma1(e, r, r);
    float a = n0 * r;
    float ea = fma1(nd, a, n0);
    a = fma1(ea, r, a);
    ea = fma1(nd, a, n0);
    q0 = fma1(ea, r, a);
    float b = n1 * r;
    float eb = fma1(nd, b, n1);
    b = fma1(eb, r, b);
    eb = fma1(nd, b, n1);
    q1 = fma1(eb, r, b);
}
DEV void visit1(const float *__restrict__ cam, float X0, float X1, float X2, float &dx, float &dy) {
    float c0 = cam[0] * X0;
    c0 = fma1(cam[1], X1, c0);
    c0 = fma1(cam[2], X2, c0);
    c0 = fma1(cam[3], 1.0f, c0);
    float c1 = cam[4] * X0;
    c1 = fma1(cam[5], X1, c1);
    c1 = fma1(cam[6], X2, c1);
    c1 = fma1(cam[7], 1.0f, c1);
    float c2 = cam[8] * X0;
    c2 = fma1(cam[9], X1, c2);
    c2 = fma1(cam[10], X2, c2);
    c2 = fma1(cam[11], 1.0f, c2);
    const float q0 = fma1(cam[18], c2, cam[16] * c0);
    const float q1 = fma1(cam[22], c2, cam[21] * c1);
    float u, v;
    div1x2(q0, q1, c2, u, v);
    const float col = (-u + 1.0f) * 32.0f, row = (v + 1.0f) * 16.0f;
    const float x0 = row - cam[12], x1 = col - cam[13];
    float s = x0 * x0;
    s = fma1(x1, x1, s);
    float nrm = sqrt_before_clamp(s);
    nrm = (nrm < 1e-8f) ? 1e-8f : nrm;
    div1x2(x0, x1, nrm, dx, dy);
}

// ---- two items on register pairs
DEV void div2x2(v2 n0, v2 n1, v2 d, v2 &q0, v2 &q1) {
    v2 r = v2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    const v2 nd = -d;
    v2 e = fma2(nd, r, splat(1.0f));
    r = fma2(e, r, r);
    v2 a = n0 * r;
    v2 ea = fma2(nd, a, n0);
    a = fma2(ea, r, a);
    ea = fma2(nd, a, n0);
    q0 = fma2(ea, r, a);
    v2 b = n1 * r;
    v2 eb = fma2(nd, b, n1);
    b = fma2(eb, r, b);
    eb = fma2(nd, b, n1);
    q1 = fma2(eb, r, b);
}
DEV void visit2(const float *__restrict__ cam, v2 X0, v2 X1, v2 X2, v2 &dx, v2 &dy) {
    v2 c0 = splat(cam[0]) * X0;
    c0 = fma2(splat(cam[1]), X1, c0);
    c0 = fma2(splat(cam[2]), X2, c0);
    c0 = fma2(splat(cam[3]), splat(1.0f), c0);
    v2 c1 = splat(cam[4]) * X0;
    c1 = fma2(splat(cam[5]), X1, c1);
    c1 = fma2(splat(cam[6]), X2, c1);
    c1 = fma2(splat(cam[7]), splat(1.0f), c1);
    v2 c2 = splat(cam[8]) * X0;
    c2 = fma2(splat(cam[9]), X1, c2);
    c2 = fma2(splat(cam[10]), X2, c2);
    c2 = fma2(splat(cam[11]), splat(1.0f), c2);
    const v2 q0 = fma2(splat(cam[18]), c2, splat(cam[16]) * c0);
    const v2 q1 = fma2(splat(cam[22]), c2, splat(cam[21]) * c1);
    v2 u, v;
    div2x2(q0, q1, c2, u, v);
    const v2 col = (-u + splat(1.0f)) * splat(32.0f), row = (v + splat(1.0f)) * splat(16.0f);
    const v2 x0 = row - splat(cam[12]), x1 = col - splat(cam[13]);
    v2 s = x0 * x0;
    s = fma2(x1, x1, s);
    v2 nrm = v2{sqrt_before_clamp(s.x), sqrt_before_clamp(s.y)};
    nrm.x = (nrm.x < 1e-8f) ? 1e-8f : nrm.x;
    nrm.y = (nrm.y < 1e-8f) ? 1e-8f : nrm.y;
    div2x2(x0, x1, nrm, dx, dy);
}

// ---- the key block: four taps (tx, ty) x four items (DX, DY), even taps into ke, odd taps into ko
#define MUL(D, A, B) asm volatile("v_mul_f32_e32 %0, %1, %2" : "=v"(D) : "v"(A), "v"(B))
#define ADD(D, A, B) asm volatile("v_add_f32_e32 %0, %1, %2" : "=v"(D) : "v"(A), "v"(B))
#define SUBC(D, X) asm volatile("v_sub_f32_e64 %0, %2, |%1|" : "=v"(D) : "v"(X), "s"(cc))
#define KEY(D, X, U) asm volatile("v_lshl_or_b32 %0, %1, 5, %2" : "=v"(D) : "v"(X), "s"(U))
#define MIN3(A, K0, K1) asm volatile("v_min3_u32 %0, %0, %1, %2" : "+v"(A) : "v"(K0), "v"(K1))
#define TAP(U, l0, l1, l2, l3, IDX) { float a0, a1, a2, a3, b0, b1, b2, b3;                                          \
      MUL(a0, tx[U], DX[0]); MUL(a1, tx[U], DX[1]); MUL(a2, tx[U], DX[2]); MUL(a3, tx[U], DX[3]);                    \
      MUL(b0, ty[U], DY[0]); MUL(b1, ty[U], DY[1]); MUL(b2, ty[U], DY[2]); MUL(b3, ty[U], DY[3]);                    \
      ADD(a0, a0, b0); ADD(a1, a1, b1); ADD(a2, a2, b2); ADD(a3, a3, b3);                                            \
      SUBC(l0, a0); SUBC(l1, a1); SUBC(l2, a2); SUBC(l3, a3);                                                        \
      KEY(l0, l0, IDX); KEY(l1, l1, IDX); KEY(l2, l2, IDX); KEY(l3, l3, IDX); }
#define KEY_BLOCK { float e0, e1, e2, e3, f0, f1, f2, f3, g0, g1, g2, g3, h0, h1, h2, h3;                            \
      TAP(0, e0, e1, e2, e3, iu) TAP(1, f0, f1, f2, f3, iu) TAP(2, g0, g1, g2, g3, iv) TAP(3, h0, h1, h2, h3, iv)    \
      MIN3(ke[0], e0, g0); MIN3(ke[1], e1, g1); MIN3(ke[2], e2, g2); MIN3(ke[3], e3, g3);                            \
      MIN3(ko[0], f0, h0); MIN3(ko[1], f1, h1); MIN3(ko[2], f2, h2); MIN3(ko[3], f3, h3); }

// the four items of a wave in one view, FORM 0 P, 1 S, 2 G; 3: no projection (the baseline of ALTERNATING)
template <int FORM>
DEV void project(const float *__restrict__ cam, float (&X0)[4], const float (&X1)[4], const float (&X2)[4], float (&DX)[4],
                 float (&DY)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(X0[j]));   // the items are not loop invariants
    if constexpr (FORM == 0) {
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {
            v2 dx, dy;
            visit2(cam, v2{X0[2 * jp], X0[2 * jp + 1]}, v2{X1[2 * jp], X1[2 * jp + 1]}, v2{X2[2 * jp], X2[2 * jp + 1]}, dx, dy);
            DX[2 * jp] = dx.x;
            DX[2 * jp + 1] = dx.y;
            DY[2 * jp] = dy.x;
            DY[2 * jp + 1] = dy.y;
        }
    } else if constexpr (FORM < 3) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (FORM == 2 && j == 2) __builtin_amdgcn_sched_barrier(0);
            visit1(cam, X0[j], X1[j], X2[j], DX[j], DY[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(DX[j]), "+v"(DY[j]));
}

// per_visit > 0: ALTERNATING, every workgroup `visits` times {project, per_visit key blocks}.  Otherwise proj_every: 1 = every
// workgroup projects, 5 = every fifth, 0 = none (the key block alone, `cap` blocks per wave); a key workgroup stops at `cap`
// blocks or, tested every 16 blocks, when `nproj` projecting workgroups have finished.
template <int FORM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void
proj_kernel(const float *__restrict__ cams, int visits, int proj_every, int per_visit, int cap, int nproj, int *done,
            unsigned long long *clk /* [WGS][2] */, unsigned *blocks /* [WGS] */, float *sink /* [WGS * 256] */, float a, float b) {
    const bool proj = per_visit || (proj_every && (blockIdx.x % proj_every == 0));
    const unsigned long long t0 = wall_clock64();
    unsigned nblk = 0;
    float X0[4], X1[4], X2[4], DX[4], DY[4], tx[4], ty[4];
    unsigned ke[4], ko[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        X0[j] = a * 0.001f * (float)(threadIdx.x + 64 * j);
        X1[j] = b * 0.002f * (float)(threadIdx.x + 3 * j);
        X2[j] = a * 0.1f * (float)j;
        DX[j] = a * 0.6f + 0.0001f * (float)(threadIdx.x + j);
        DY[j] = b * 0.8f - 0.0001f * (float)(threadIdx.x + j);
        tx[j] = a * (0.5f + 0.1f * (float)j);
        ty[j] = b * (0.8f - 0.1f * (float)j);
        ke[j] = ko[j] = 0xFFFFFFFFu;
    }
    const float cc = a + 6.1035156e-05f;
    const unsigned iu = (unsigned)blockIdx.x & 15u, iv = iu + 16u;
    if (per_visit) {
        const int ahead = (int)(blockIdx.x % 5) * per_visit / 5;
#pragma unroll 1
        for (int k = 0; k < ahead; ++k) KEY_BLOCK
        for (int i = 0; i < visits; ++i) {
            project<FORM>(cams + (i & 7) * CAM, X0, X1, X2, DX, DY);
#pragma unroll 1
            for (int k = 0; k < per_visit; ++k) KEY_BLOCK
        }
        nblk = (unsigned)(ahead + visits * per_visit);
    } else if (proj) {
        for (int i = 0; i < visits; ++i) project<FORM>(cams + (i & 7) * CAM, X0, X1, X2, DX, DY);
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(done, 1);
    } else {
        for (int n = 0; n < cap; n += 16) {
#pragma unroll 1
            for (int k = 0; k < 16; ++k) KEY_BLOCK
            nblk += 16;
            if (__atomic_load_n(done, __ATOMIC_RELAXED) >= nproj) break;
        }
    }
    const unsigned long long t1 = wall_clock64();
    sink[blockIdx.x * 256 + threadIdx.x] = DX[0] + DY[3] + __uint_as_float((ke[0] ^ ke[1] ^ ke[2] ^ ke[3]) + (ko[0] ^ ko[1] ^ ko[2] ^ ko[3]));
    if (threadIdx.x == 0) {
        clk[2 * blockIdx.x] = t0;
        clk[2 * blockIdx.x + 1] = t1;
        blocks[blockIdx.x] = nblk;
    }
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct Result {
    double launch_ns;      // first start to last end of the projecting workgroups (of all workgroups when none projects)
    double wave_ns;        // mean duration of a projecting workgroup
    double key_blocks;     // wave-level key blocks done, all key waves together
};

template <int FORM>
int run(const float *d_cams, int visits, int proj_every, int per_visit, int cap, int *d_done, unsigned long long *d_clk, unsigned *d_blocks,
        float *d_sink, double tick_ns, Result &res) {
    int nproj = 0;
    for (int w = 0; w < WGS; ++w) nproj += (per_visit || (proj_every && w % proj_every == 0)) ? 1 : 0;
    std::vector<unsigned long long> clk(2 * WGS);
    std::vector<unsigned> blocks(WGS);
    for (int rep = 0; rep < 2; ++rep) {   // the first launch warms up
        CHECK(hipMemset(d_done, 0, sizeof(int)));
        hipLaunchKernelGGL(proj_kernel<FORM>, dim3(WGS), dim3(256), 0, 0, d_cams, visits, proj_every, per_visit, cap,
                           proj_every ? nproj : 0x7fffffff, d_done, d_clk, d_blocks, d_sink, 1.0f, 0.999f);
        CHECK(hipDeviceSynchronize());
    }
    CHECK(hipMemcpy(clk.data(), d_clk, sizeof(unsigned long long) * 2 * WGS, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(blocks.data(), d_blocks, sizeof(unsigned) * WGS, hipMemcpyDeviceToHost));
    unsigned long long first = ~0ull, last = 0;
    double sum = 0.0;
    res.key_blocks = 0.0;
    for (int w = 0; w < WGS; ++w) {
        const bool proj = per_visit || (proj_every && w % proj_every == 0);
        if (proj || !proj_every) {
            first = clk[2 * w] < first ? clk[2 * w] : first;
            last = clk[2 * w + 1] > last ? clk[2 * w + 1] : last;
        }
        if (proj) sum += (double)(clk[2 * w + 1] - clk[2 * w]);
        res.key_blocks += 4.0 * blocks[w];
    }
    res.launch_ns = (double)(last - first) * tick_ns;
    res.wave_ns = nproj ? sum / nproj * tick_ns : 0.0;
    return 0;
}

int main() {
    int rate_khz = 0;
    CHECK(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, 0));
    const double tick_ns = 1e6 / (double)rate_khz;
    float cams[8 * CAM];
    for (int v = 0; v < 8; ++v) {
        float *c = cams + v * CAM;
        for (int i = 0; i < CAM; ++i) c[i] = 0.0f;
        c[0] = 1.0f; c[1] = 0.01f * v; c[3] = 0.1f;            // camera-space x
        c[5] = 1.0f; c[6] = 0.02f; c[7] = -0.1f;               // camera-space y
        c[8] = 0.05f; c[10] = 0.3f; c[11] = 2.0f + 0.1f * v;   // depth, 2 .. 3
        c[16] = 1.5f; c[18] = 0.01f; c[21] = 1.5f; c[22] = -0.01f;
        c[12] = 15.5f; c[13] = 31.5f;                          // patch centre (row, col)
    }
    float *d_cams, *d_sink;
    int *d_done;
    unsigned long long *d_clk;
    unsigned *d_blocks;
    CHECK(hipMalloc(&d_cams, sizeof(cams)));
    CHECK(hipMemcpy(d_cams, cams, sizeof(cams), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d_sink, sizeof(float) * WGS * 256));
    CHECK(hipMalloc(&d_done, sizeof(int)));
    CHECK(hipMalloc(&d_clk, sizeof(unsigned long long) * 2 * WGS));
    CHECK(hipMalloc(&d_blocks, sizeof(unsigned) * WGS));

    const int visits = 4000, key_cap = 1 << 17;   // (the cap: ~0.05 s of key blocks, not reached)
    printf("wall clock %d kHz; %d workgroups x 256 lanes, 5 waves per SIMD; %d visits of 4 items per projecting wave\n", rate_khz, WGS, visits);
    Result key;
    if (run<0>(d_cams, 0, 0, 0, 16000, d_done, d_clk, d_blocks, d_sink, tick_ns, key)) return 1;
    const double block_simd_ns = key.launch_ns * SIMDS / key.key_blocks;
    printf("key block alone, 5 waves per SIMD: %.0f wave-blocks in %.1f us: %.2f ns = %.1f cycles@2.4GHz of SIMD time per block of 4 taps x 4 items\n",
           key.key_blocks, key.launch_ns * 1e-3, block_simd_ns, block_simd_ns * 2.4);
    const char *names[3] = {"P two packed pairs", "S four plain chains", "G plain, two by two"};
    for (int mixed = 0; mixed < 2; ++mixed) {
        for (int form = 0; form < 3; ++form) {
            Result r;
            const int every = mixed ? 5 : 1;
            int rc = form == 0 ? run<0>(d_cams, visits, every, 0, key_cap, d_done, d_clk, d_blocks, d_sink, tick_ns, r)
                   : form == 1 ? run<1>(d_cams, visits, every, 0, key_cap, d_done, d_clk, d_blocks, d_sink, tick_ns, r)
                               : run<2>(d_cams, visits, every, 0, key_cap, d_done, d_clk, d_blocks, d_sink, tick_ns, r);
            if (rc) return 1;
            const double wave = r.wave_ns / visits;
            if (!mixed)
                printf("ALONE       %-20s per (wave, view) visit: wave %7.1f ns = %6.0f cycles | SIMD %6.1f ns = %5.0f cycles@2.4GHz  (launch %.1f us)\n",
                       names[form], wave, wave * 2.4, wave / 5.0, wave / 5.0 * 2.4, r.launch_ns * 1e-3);
            else
                printf("MIXED       %-20s per (wave, view) visit: wave %7.1f ns = %6.0f cycles | beside it %.0f key wave-blocks in %.1f us: %.2f ns of SIMD "
                       "time per block\n", names[form], wave, wave * 2.4, r.key_blocks, r.launch_ns * 1e-3, r.launch_ns * SIMDS / r.key_blocks);
        }
    }
    const int alt_visits = 2000, per_visit = 12;
    Result base;
    if (run<3>(d_cams, alt_visits, 0, per_visit, 0, d_done, d_clk, d_blocks, d_sink, tick_ns, base)) return 1;
    printf("ALTERNATING no projection    %d x %d key blocks per wave: launch %.1f us: %.2f ns of SIMD time per block\n", alt_visits, per_visit,
           base.launch_ns * 1e-3, base.launch_ns * SIMDS / base.key_blocks);
    for (int form = 0; form < 3; ++form) {
        Result r;
        int rc = form == 0 ? run<0>(d_cams, alt_visits, 0, per_visit, 0, d_done, d_clk, d_blocks, d_sink, tick_ns, r)
               : form == 1 ? run<1>(d_cams, alt_visits, 0, per_visit, 0, d_done, d_clk, d_blocks, d_sink, tick_ns, r)
                           : run<2>(d_cams, alt_visits, 0, per_visit, 0, d_done, d_clk, d_blocks, d_sink, tick_ns, r);
        if (rc) return 1;
        const double simd = (r.launch_ns - base.launch_ns) / alt_visits / 5.0;
        printf("ALTERNATING %-20s per (wave, view) visit: SIMD %6.1f ns = %5.0f cycles@2.4GHz  (launch %.1f us, %.1f us over no projection)\n",
               names[form], simd, simd * 2.4, r.launch_ns * 1e-3, (r.launch_ns - base.launch_ns) * 1e-3);
    }
    return 0;
}
