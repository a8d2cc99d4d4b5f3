// Wave-level primitives of the gfx950 kernels (wave64): DPP row rotations, lane reads and writes, wave-uniform values in SGPRs, the wave sum / maximum of
// the solver's workgroup object (unevenhip.hip DevWG) and the selection reductions of the trajectory queries (traj_query.hip).
#pragma once
#include <hip/hip_runtime.h>

// wave64 sum with DPP row rotations (no LDS traffic, no barrier): rotate-and-add inside each row of 16 lanes, then the four
// row totals are read from lanes 0/16/32/48 and added in a fixed order, so every lane gets the same bits.
template <int CTRL>
__device__ __forceinline__ double dppMov(double v) {
    // a row rotation writes every lane, so no "old" value has to be preserved: mov_dpp (undefined old) spares the two copies
    // per step that update_dpp(old = src) costs on the dependency chain of every reduction
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readLane(double v, int l) {      // l must be wave-uniform
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// wave-uniform values (block reduction results, ring positions, ...) are moved to SGPRs explicitly: the compiler cannot prove
// uniformity of anything that passed through LDS, and would otherwise keep loop bounds in VGPRs, branch through exec masks and
// -- worst -- park them in scratch, whose reload forces s_waitcnt vmcnt(0) and drains every prefetch in flight.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uni(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
typedef const __attribute__((address_space(1))) double* gcptr;       // read-only global pointer
__device__ __forceinline__ gcptr uniG(const double* p) {             // wave-uniform global pointer held in an SGPR pair
    const unsigned long long a = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return (gcptr)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double writeLane(double v /*wave-uniform*/, int l /*wave-uniform*/, double old) {   // old with lane l replaced by v
    int hi = __double2hiint(old), lo = __double2loint(old);
    const int vh = __builtin_amdgcn_readfirstlane(__double2hiint(v)), vl = __builtin_amdgcn_readfirstlane(__double2loint(v));
    const int ls = __builtin_amdgcn_readfirstlane(l);
    asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(hi) : "s"(vh), "s"(ls) : "m0");
    asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(lo) : "s"(vl), "s"(ls) : "m0");
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double waveSum(double v) {
    v += dppMov<0x128>(v);   // row_ror:8
    v += dppMov<0x124>(v);   // row_ror:4
    v += dppMov<0x122>(v);   // row_ror:2
    v += dppMov<0x121>(v);   // row_ror:1
    return ((readLane(v, 0) + readLane(v, 16)) + readLane(v, 32)) + readLane(v, 48);
}

__device__ __forceinline__ double waveMax(double v) {
    double o;
    o = dppMov<0x128>(v); v = o > v ? o : v;
    o = dppMov<0x124>(v); v = o > v ? o : v;
    o = dppMov<0x122>(v); v = o > v ? o : v;
    o = dppMov<0x121>(v); v = o > v ? o : v;
    const double a = readLane(v, 0), b = readLane(v, 16), c = readLane(v, 32), d = readLane(v, 48);
    const double ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}
template <int CTRL>
__device__ __forceinline__ int dppMovI(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, false); }

// ---- reductions of a few values per lane under an operation whose result does not depend on the order of combination (a selection under a total order, an
// integer sum): op(v..., o...) folds the values o... of another lane into this lane's v....  Values are double, int or unsigned long long.
template <int CTRL>
__device__ __forceinline__ int dppMov(int v) { return dppMovI<CTRL>(v); }
template <int CTRL>
__device__ __forceinline__ unsigned long long dppMov(unsigned long long v) {
    const unsigned lo = (unsigned)dppMovI<CTRL>((int)(unsigned)v), hi = (unsigned)dppMovI<CTRL>((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ int readLane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ unsigned long long readLane(unsigned long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}
template <int CTRL, class Op, class... T>
__device__ __forceinline__ void rowStep(Op op, T&... v) { op(v..., dppMov<CTRL>(v)...); }
// inside each row of 16 lanes: afterwards every lane holds its row's result
template <class Op, class... T>
__device__ __forceinline__ void rowReduce(Op op, T&... v) { rowStep<0x128>(op, v...); rowStep<0x124>(op, v...); rowStep<0x122>(op, v...); rowStep<0x121>(op, v...); }
// the four rows of the wave, read from lanes 0 / 16 / 32 / 48 and folded in that order: afterwards v... is the wave's result, wave-uniform
template <class Op, class... T>
__device__ __forceinline__ void rowLeaders(Op op, T&... v) {
    [&](T... row) {
        ((v = readLane(row, 0)), ...);
#pragma unroll
        for (int r = 16; r < 64; r += 16) op(v..., readLane(row, r)...);
    }(v...);
}
// across the NW waves of the workgroup: every wave leaves its result in lds (one array of NW per value, in argument order -- the caller lists the 8-byte
// values first and provides NW * the values' sizes), a barrier, thread 0 folds waves 1 .. NW - 1 into its own in that order.  wavesFold / acrossWaves
// return whether this thread holds the workgroup's result (thread 0 alone).  NW = 1: no LDS, no barrier.
template <int NW, class... T>
__device__ __forceinline__ void wavesPut(void* lds, T... v) {
    char* p = (char*)lds;
    if (NW > 1 && (threadIdx.x & 63) == 0) (((((T*)p)[threadIdx.x >> 6] = v), p += NW * sizeof(T)), ...);
}
template <int NW, class Op, class... T>
__device__ __forceinline__ bool wavesFold(Op op, const void* lds, T&... v) {
    if (NW > 1 && threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < NW; w++) {
            [&](T... o) {
                const char* p = (const char*)lds;
                (((o = ((const T*)p)[w]), p += NW * sizeof(T)), ...);
                op(v..., o...);
            }(v...);
        }
    }
    return threadIdx.x == 0;
}
template <int NW, class Op, class... T>
__device__ __forceinline__ bool acrossWaves(Op op, void* lds, T&... v) {
    wavesPut<NW>(lds, v...);
    if (NW > 1) __syncthreads();
    return wavesFold<NW>(op, lds, v...);
}
// the bytes wavesPut<NW> writes for values of types T..., and whether they are listed widest first
template <class... T>
constexpr int wavesBytes(int nw) { return nw * (int)(sizeof(T) + ...); }
template <class... T>
constexpr bool wavesOrdered() {
    size_t prev = 8;
    bool ok = true;
    ((ok = ok && sizeof(T) <= prev, prev = sizeof(T)), ...);
    return ok;
}
// the whole reduction over a workgroup of NT lanes, with the LDS it needs: rows, row leaders, waves.  Returns whether this thread holds the result (thread 0).
// The array belongs to the instantiation <NT, Op, T...>: a kernel that makes the same call twice needs a barrier between the two (the second call's waves
// would write the slots thread 0 may still be folding); no kernel does so today.
template <int NT, class Op, class... T>
__device__ __forceinline__ bool workgroupReduce(Op op, T&... v) {
    static_assert(NT % 64 == 0 && wavesOrdered<T...>(), "whole waves; the 8-byte values first");
    __shared__ double lds[(wavesBytes<T...>(NT / 64) + 7) / 8];
    rowReduce(op, v...);
    rowLeaders(op, v...);
    return acrossWaves<NT / 64>(op, lds, v...);
}
