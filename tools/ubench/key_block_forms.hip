// Micro-benchmark (gfx950): one (wave, view) visit of the one-group key kernels of csrc/pmvo_search.hip -- a 49-tap list (7 x 7 patch)
// in LDS, FOUR items per lane: the seeded last tap, twelve four-tap blocks, the decode -- in three forms, on the blocks of
// csrc/mh_key_blocks.h itself and of tools/gen_key_blocks.py --form sub4:
//   T  the per-TAP keys: key = (t' << 5) | place, even taps into one accumulator and odd taps into another (mh_key_block4), the two
//      merged after the walk, the winner's confidence read from its record
//   M  the per-BLOCK keys: m = min of the block's four t', key = (m << 4) | block, one accumulator (the block of --form sub4: four
//      subtractions, v_min_u32, v_min3_u32); after the walk every lane reads ITS winning block's (tx, ty) again, makes the t' again
//      and takes the first that equals m
//   X  the same with the MAXIMUM first: m = C - max of the block's four |cs| (mh_key_blockm4 as committed: v_max_f32, v_max3_f32
//      with |.| on the sources, one subtraction); the rest is M's
//   W  X with the twelve blocks as straight-line code (mh_key_walk<12>: the block numbers, the parities and the offsets of the taps
//      are constants, no loop, no key copied between the two variants of the block); seed and decode are X's
// The taps are unit vectors at the angles pi * t / 49, the items' directions are spread over the half circle lane by lane, so that the
// winning blocks differ among the lanes of a wave (the per-lane LDS reads of M go to twelve or more different blocks; printed).  Both
// forms add loss * confidence and confidence over the visits; the sums are compared bit for bit (T with M, M with X, X with W).
// 5 waves per SIMD (1280 workgroups of 256 lanes).  ALONE: every wave visits, back to back.  ALTERNATING: every wave projects its four
// items (the plain chains of tools/ubench/proj_forms.hip, form S) and then visits, the workgroups starting 0, 2, 4, 7 and 9 blocks into
// that cycle, so that a wave in its decode runs beside waves in their key blocks and in their projection.
// Prints SIMD time per (wave, view) visit = launch time / visits / 5 waves, in ns and in cycles at an assumed 2.4 GHz: median and spread
// (max - min) of REPS launches behind WARM that warm up.
//   python tools/gen_key_blocks.py --form sub4 --only-blockm4 --name mh_key_blockm4_sub4 > /tmp/sub4.h
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -DKEY_BLOCKS_SUB4_H='"/tmp/sub4.h"' \
//         -o /tmp/key_block_forms tools/ubench/key_block_forms.hip
// Another interleave of mh_key_blockm4 (tools/gen_key_blocks.py --width W > /tmp/w.h): add -DKEY_BLOCKS_H='"/tmp/w.h"'.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#define MH_KEY_C 1.00006103515625f   // 1 + 2^-14
#define MH_KEY_E 6.103515625e-05f
#ifndef KEY_BLOCKS_H
#define KEY_BLOCKS_H "../../monohair_amd/csrc/mh_key_blocks.h"
#endif
#include KEY_BLOCKS_H
#ifndef KEY_BLOCKS_SUB4_H
#error "KEY_BLOCKS_SUB4_H: the header of tools/gen_key_blocks.py --form sub4 --only-blockm4 --name mh_key_blockm4_sub4"
#endif
#include KEY_BLOCKS_SUB4_H

#define WGS 1280     // 256 CUs x 5 workgroups: 5 waves on every SIMD
#define NTAP 49
#define REPS 7
#define WARM 3    // launches in front of them: the first ones of a form run at another clock
#define CAM 24
#define DEV __device__ __forceinline__
typedef float v2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(3))) v2 *lds_v2;
typedef const __attribute__((address_space(3))) float *lds_f1;

DEV float vmul(float a, float b) { float d; asm("v_mul_f32_e32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
DEV float vadd(float a, float b) { float d; asm("v_add_f32_e32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
DEV float tprime(float cs) { float t; asm("v_sub_f32_e64 %0, %2, |%1|" : "=v"(t) : "v"(cs), "s"(MH_KEY_C)); return t; }
DEV unsigned keyof(float t, int sh5, int idx) {
    unsigned k;
    if (sh5) asm("v_lshl_or_b32 %0, %1, 5, %2" : "=v"(k) : "v"(t), "s"(idx));
    else asm("v_lshl_or_b32 %0, %1, 4, %2" : "=v"(k) : "v"(t), "s"(idx));
    return k;
}

// ---- the projection of one item (proj_forms.hip, form S)
DEV float fma1(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
DEV float sqrt_before_clamp(float x) {
    float r = __builtin_amdgcn_sqrtf(x);
    const float rd = __uint_as_float(__float_as_uint(r) - 1u), ru = __uint_as_float(__float_as_uint(r) + 1u);
    const float ed = fma1(-rd, r, x), eu = fma1(-ru, r, x);
    r = (0.0f >= ed) ? rd : r;
    r = (0.0f < eu) ? ru : r;
    return r;
}
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

// ---- one visit, form T: rec = the list in LDS (header, taps); the first nblk blocks are walked (12: the whole list)
DEV void visit_T(const float4 *rec, int nblk, const float (&DX)[4], const float (&DY)[4], float (&ML)[4], float (&BC)[4]) {
    const int ntp = 4 * nblk;
    unsigned ke[4], ko[4];
    const unsigned rec1 = (unsigned)(size_t)(const __attribute__((address_space(3))) float4 *)(rec + 1);
    const float2 *__restrict__ t2 = reinterpret_cast<const float2 *>(rec + 1);
    float2 ga[4], gb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) ga[u] = t2[2 * u];
    const int is = NTAP - 1;
    const float2 ts = t2[2 * is];
    const bool even = (is & 1) == 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned k = keyof(tprime(vadd(vmul(ts.x, DX[j]), vmul(ts.y, DY[j]))), 1, is >> 1);
        ke[j] = even ? k : 0xFFFFFFFFu;
        ko[j] = even ? 0xFFFFFFFFu : k;
    }
    for (int t = 0; t < ntp;) {
#pragma unroll
        for (int u = 0; u < 4; ++u) gb[u] = t2[2 * (t + 4 + u)];
        mh_key_block4<4, 4>(ke, ko, ga, DX, DY, t >> 1);
        t += 4;
        if (t >= ntp) break;
#pragma unroll
        for (int u = 0; u < 4; ++u) ga[u] = t2[2 * (t + 4 + u)];
        mh_key_block4<4, 4>(ke, ko, gb, DX, DY, t >> 1);
        t += 4;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool odd = ko[j] < ke[j];
        const unsigned kb = odd ? ko[j] : ke[j];
        const unsigned ad = rec1 + ((kb & 31u) << 5) + (odd ? 16u : 0u);
        BC[j] = *reinterpret_cast<lds_f1>((size_t)(ad + 8u));
        ML[j] = __uint_as_float(__builtin_amdgcn_alignbit(7u, kb, 5u)) - MH_KEY_E;
    }
}

// ---- one visit, form M (MAXF = false), X (MAXF = true) or W (MAXF and WALK; the walk is the whole list's, so the short first
// visit that staggers the workgroups keeps the loop); blk[j] = the winning block of item j
template <bool MAXF, bool WALK = false>
DEV void visit_M(const float4 *rec, int nblk, const float (&DX)[4], const float (&DY)[4], float (&ML)[4], float (&BC)[4], unsigned (&blk)[4]) {
    const int ntp = 4 * nblk;
    unsigned acc[4], kk[4];
    const unsigned rec1 = (unsigned)(size_t)(const __attribute__((address_space(3))) float4 *)(rec + 1);
    const float2 *__restrict__ t2 = reinterpret_cast<const float2 *>(rec + 1);
    float2 ga[4], gb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) ga[u] = t2[2 * u];
    const int is = NTAP - 1;
    const float2 ts = t2[2 * is];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = keyof(tprime(vadd(vmul(ts.x, DX[j]), vmul(ts.y, DY[j]))), 0, is >> 2);
    if (WALK && nblk == 12) mh_key_walk<12, 4, 4>(acc, ga, t2, DX, DY);
    else
    for (int t = 0; t < ntp;) {
#pragma unroll
        for (int u = 0; u < 4; ++u) gb[u] = t2[2 * (t + 4 + u)];
        if constexpr (MAXF) mh_key_blockm4<4, 4, false>(acc, kk, ga, DX, DY, t >> 2);
        else mh_key_blockm4_sub4<4, 4, false>(acc, kk, ga, DX, DY, t >> 2);
        t += 4;
        if (t >= ntp) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = min(acc[j], kk[j]);
            break;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) ga[u] = t2[2 * (t + 4 + u)];
        if constexpr (MAXF) mh_key_blockm4<4, 4, true>(acc, kk, gb, DX, DY, t >> 2);
        else mh_key_blockm4_sub4<4, 4, true>(acc, kk, gb, DX, DY, t >> 2);
        t += 4;
    }
#pragma unroll
    for (int j0 = 0; j0 < 4; j0 += 2) {
        if (j0) __builtin_amdgcn_sched_barrier(0);
        unsigned ad[2], mb[2];
        v2 w[2][3];
#pragma unroll
        for (int j = j0; j < j0 + 2; ++j) {
            blk[j] = acc[j] & 15u;
            ad[j - j0] = rec1 + (blk[j] << 6);
            mb[j - j0] = __builtin_amdgcn_alignbit(3u, acc[j], 4u);
#pragma unroll
            for (int u = 0; u < 3; ++u) w[j - j0][u] = *reinterpret_cast<lds_v2>((size_t)(ad[j - j0] + 16u * u));
        }
#pragma unroll
        for (int j = j0; j < j0 + 2; ++j) {
            unsigned off = 56u;
#pragma unroll
            for (int u = 2; u >= 0; --u) {
                const v2 tp = w[j - j0][u];
                const float tq = tprime(vadd(vmul(tp.x, DX[j]), vmul(tp.y, DY[j])));
                off = (__float_as_uint(tq) == mb[j - j0]) ? 8u + 16u * u : off;
            }
            BC[j] = *reinterpret_cast<lds_f1>((size_t)(ad[j - j0] + off));
            ML[j] = __uint_as_float(mb[j - j0]) - MH_KEY_E;
        }
    }
}

// FORM 0 T, 1 M, 2 X, 3 W.  PROJ: every visit is preceded by the projection of the wave's four items.
template <int FORM, bool PROJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void
visit_kernel(const float *__restrict__ cams, const float4 *__restrict__ list /* [1 + NTAP + 7] */, int visits,
             unsigned long long *clk /* [WGS][2] */, float *sums /* [256][4][2] of workgroup 0 */, unsigned *blocks /* [256][4] */, float a, float b) {
    __shared__ float4 s_taps[1 + NTAP + 7];
    if (threadIdx.x < 1 + NTAP + 7) s_taps[threadIdx.x] = list[threadIdx.x];
    __syncthreads();
    const unsigned long long t0 = wall_clock64();
    float X0[4], X1[4], X2[4], DX[4], DY[4], num[4], den[4], px = 0.0f;
    unsigned blk[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        X0[j] = a * 0.001f * (float)(threadIdx.x + 64 * j);
        X1[j] = b * 0.002f * (float)(threadIdx.x + 3 * j);
        X2[j] = a * 0.1f * (float)j;
        // the items' directions: over the half circle lane by lane, the four items of a lane a quarter of it apart
        const float phi = a * 3.14159265f * ((float)((threadIdx.x & 63) * 4 + j * 67 + 1) / 256.0f);
        DX[j] = __cosf(phi);
        DY[j] = __sinf(phi);
        num[j] = den[j] = 0.0f;
    }
    const int ahead = PROJ ? (int)(blockIdx.x % 5) * 12 / 5 : 0;
    for (int i = 0; i < visits + (ahead ? 1 : 0); ++i) {
        if constexpr (PROJ) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                asm volatile("" : "+v"(X0[j]));
                float dx, dy;
                visit1(cams + (i & 7) * CAM, X0[j], X1[j], X2[j], dx, dy);
                px += dx + dy;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(DX[j]), "+v"(DY[j]));
        float ML[4], BC[4];
        const int nblk = (ahead && i == 0) ? ahead : 12;   // (the first, short walk only staggers the workgroups)
        if constexpr (FORM == 0) visit_T(s_taps, nblk, DX, DY, ML, BC);
        else visit_M<FORM >= 2, FORM == 3>(s_taps, nblk, DX, DY, ML, BC, blk);
        if (!(ahead && i == 0)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                num[j] = num[j] + ML[j] * BC[j];
                den[j] = den[j] + BC[j];
            }
        }
    }
    const unsigned long long t1 = wall_clock64();
    if (blockIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sums[(threadIdx.x * 4 + j) * 2] = num[j];
            sums[(threadIdx.x * 4 + j) * 2 + 1] = den[j];
            blocks[threadIdx.x * 4 + j] = blk[j];
        }
    }
    if (px == 12345.678f) sums[0] = px;   // (keeps the projection)
    if (threadIdx.x == 0) {
        clk[2 * blockIdx.x] = t0;
        clk[2 * blockIdx.x + 1] = t1;
    }
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct Bufs {
    float *cams;
    float4 *list;
    unsigned long long *clk;
    float *sums;
    unsigned *blocks;
};

// median and spread of the SIMD time per visit [ns] over REPS launches behind WARM more; the sums and blocks of workgroup 0
template <int FORM, bool PROJ>
int run(const Bufs &d, int visits, double tick_ns, double &med, double &spread, std::vector<float> &sums, std::vector<unsigned> &blocks) {
    std::vector<unsigned long long> clk(2 * WGS);
    std::vector<double> ns;
    for (int rep = 0; rep < WARM + REPS; ++rep) {
        hipLaunchKernelGGL((visit_kernel<FORM, PROJ>), dim3(WGS), dim3(256), 0, 0, d.cams, d.list, visits, d.clk, d.sums, d.blocks, 1.0f, 0.999f);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(clk.data(), d.clk, sizeof(unsigned long long) * 2 * WGS, hipMemcpyDeviceToHost));
        unsigned long long first = ~0ull, last = 0;
        for (int w = 0; w < WGS; ++w) {
            first = std::min(first, clk[2 * w]);
            last = std::max(last, clk[2 * w + 1]);
        }
        if (rep >= WARM) ns.push_back((double)(last - first) * tick_ns / visits / 5.0);
    }
    std::sort(ns.begin(), ns.end());
    med = ns[ns.size() / 2];
    spread = ns.back() - ns.front();
    sums.resize(256 * 4 * 2);
    blocks.resize(256 * 4);
    CHECK(hipMemcpy(sums.data(), d.sums, sizeof(float) * sums.size(), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(blocks.data(), d.blocks, sizeof(unsigned) * blocks.size(), hipMemcpyDeviceToHost));
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
        c[0] = 1.0f; c[1] = 0.01f * v; c[3] = 0.1f;
        c[5] = 1.0f; c[6] = 0.02f; c[7] = -0.1f;
        c[8] = 0.05f; c[10] = 0.3f; c[11] = 2.0f + 0.1f * v;
        c[16] = 1.5f; c[18] = 0.01f; c[21] = 1.5f; c[22] = -0.01f;
        c[12] = 15.5f; c[13] = 31.5f;
    }
    // the list: header, 49 unit taps at the angles pi * t / 49 with a confidence of their own, zero records behind them
    float4 list[1 + NTAP + 7];
    memset(list, 0, sizeof(list));
    for (int t = 0; t < NTAP; ++t) {
        const double th = 3.14159265358979 * t / NTAP;
        list[1 + t] = make_float4((float)cos(th), (float)sin(th), 0.25f + (float)t / 128.0f, 0.0f);
    }
    Bufs d;
    CHECK(hipMalloc(&d.cams, sizeof(cams)));
    CHECK(hipMemcpy(d.cams, cams, sizeof(cams), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d.list, sizeof(list)));
    CHECK(hipMemcpy(d.list, list, sizeof(list), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&d.clk, sizeof(unsigned long long) * 2 * WGS));
    CHECK(hipMalloc(&d.sums, sizeof(float) * 256 * 4 * 2));
    CHECK(hipMalloc(&d.blocks, sizeof(unsigned) * 256 * 4));

    const int visits = 2000;
    printf("wall clock %d kHz; %d workgroups x 256 lanes, 5 waves per SIMD; %d visits of 4 items x (seed + 12 blocks + decode) per wave; %d launches each\n",
           rate_khz, WGS, visits, REPS);
    double med[2][4], spr[2][4];
    std::vector<float> sums[2][4];
    std::vector<unsigned> blocks[2][4];
    if (run<0, false>(d, visits, tick_ns, med[0][0], spr[0][0], sums[0][0], blocks[0][0])) return 1;
    if (run<1, false>(d, visits, tick_ns, med[0][1], spr[0][1], sums[0][1], blocks[0][1])) return 1;
    if (run<2, false>(d, visits, tick_ns, med[0][2], spr[0][2], sums[0][2], blocks[0][2])) return 1;
    if (run<3, false>(d, visits, tick_ns, med[0][3], spr[0][3], sums[0][3], blocks[0][3])) return 1;
    if (run<0, true>(d, visits, tick_ns, med[1][0], spr[1][0], sums[1][0], blocks[1][0])) return 1;
    if (run<1, true>(d, visits, tick_ns, med[1][1], spr[1][1], sums[1][1], blocks[1][1])) return 1;
    if (run<2, true>(d, visits, tick_ns, med[1][2], spr[1][2], sums[1][2], blocks[1][2])) return 1;
    if (run<3, true>(d, visits, tick_ns, med[1][3], spr[1][3], sums[1][3], blocks[1][3])) return 1;
    const char *mode[2] = {"ALONE      ", "ALTERNATING"}, *form[4] = {"T per-tap keys  ", "M per-block keys", "X maximum first ", "W straight walk "};
    const char *nm = "TMXW";
    for (int p = 0; p < 2; ++p)
        for (int f = 0; f < 4; ++f)
            printf("%s %s per (wave, view) visit%s: SIMD %7.2f ns = %6.1f cycles@2.4GHz, spread %.2f ns\n", mode[p], form[f],
                   p ? " with its projection" : "", med[p][f], med[p][f] * 2.4, spr[p][f]);
    for (int p = 0; p < 2; ++p)
        for (int f = 1; f < 4; ++f) {   // M against T, X against M, W against X
            const double gain = med[p][f - 1] - med[p][f], noise = std::max(spr[p][f - 1], spr[p][f]);
            printf("%s %c is %+.2f ns = %+.1f cycles (%+.1f %%) against %c; larger spread %.2f ns: %s\n", mode[p], nm[f], -gain, -gain * 2.4,
                   -100.0 * gain / med[p][f - 1], nm[f - 1], noise, gain > noise ? "cheaper by more than the spread" : "NOT cheaper by more than the spread");
        }
    bool same = true;
    for (int p = 0; p < 2; ++p)
        for (int f = 1; f < 4; ++f) same = same && memcmp(sums[p][0].data(), sums[p][f].data(), sizeof(float) * sums[p][0].size()) == 0;
    bool same_blocks = true;
    for (int p = 0; p < 2; ++p) same_blocks = same_blocks && blocks[p][1] == blocks[p][2] && blocks[p][2] == blocks[p][3];
    int distinct = 0;
    {
        bool seen[16] = {};
        for (int l = 0; l < 64; ++l) seen[blocks[0][1][l * 4] & 15u] = true;   // item 0 of the lanes of wave 0
        for (int i = 0; i < 16; ++i) distinct += seen[i] ? 1 : 0;
    }
    printf("sums of loss * confidence and of confidence, 1024 items of workgroup 0: T, M, X and W %s; winning blocks of M, X and W %s; winning blocks of item 0 among the 64 lanes of wave 0: %d different\n",
           same ? "bit-equal" : "DIFFER", same_blocks ? "equal" : "DIFFER", distinct);
    return same && same_blocks ? 0 : 2;
}
