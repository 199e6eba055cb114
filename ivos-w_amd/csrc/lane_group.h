// What the streaming "session glue" kernels (qa, seg_epilogue, atnet_epilogue, ipn_glue, overlay, scribble) share: a lane owns a GROUP of
// V consecutive elements and moves it with one aligned access, and the launcher picks the widest V whose accesses all lie on their grids.
//   device half  load_group / store_group / store_group_as / store_bytes on plain arrays: the kernels keep their arithmetic, the vector
//                types and the byte packing live here.  HIP's float4 / uint4 into arrays, not clang ext_vector_type (LAB_NOTES.md: the
//                latter cost two VGPRs in dqn_update.h).
//   host half    scalar_forced / on_grid / multiples_of state the launchers' predicate once; lane_blocks and dispatch_lanes turn the V
//                they choose into grid.x and the kernel<V> that runs.
#pragma once
#include <assert.h>
#include <stdlib.h>

#include <type_traits>

#include "common.h"

namespace ivosw {

// ---------------------------------------------------------------- device half
template <class T> struct GroupVec;
template <> struct GroupVec<float> { using two = float2; using four = float4; };
template <> struct GroupVec<uint32_t> { using two = uint2; using four = uint4; };

// v = p[0 .. V): ONE aligned access of 4 V bytes for V = 1, 2, 4 (p on the 4 V-byte grid); V = 16 is four 16-byte accesses
template <class T, int V>
__device__ __forceinline__ void load_group(const T* p, T (&v)[V]) {
    static_assert(V == 1 || V == 2 || V % 4 == 0, "a group is 1, 2 or a multiple of 4 elements");
    if constexpr (V == 1) {
        v[0] = *p;
    } else if constexpr (V == 2) {
        const auto q = *reinterpret_cast<const typename GroupVec<T>::two*>(p);
        v[0] = q.x; v[1] = q.y;
    } else {
#pragma unroll
        for (int j = 0; j < V; j += 4) {
            const auto q = *reinterpret_cast<const typename GroupVec<T>::four*>(p + j);
            v[j] = q.x; v[j + 1] = q.y; v[j + 2] = q.z; v[j + 3] = q.w;
        }
    }
}

template <class T, int V>
__device__ __forceinline__ void store_group(T* p, const T (&v)[V]) {
    static_assert(V == 1 || V == 2 || V % 4 == 0, "a group is 1, 2 or a multiple of 4 elements");
    if constexpr (V == 1) {
        *p = v[0];
    } else if constexpr (V == 2) {
        *reinterpret_cast<typename GroupVec<T>::two*>(p) = typename GroupVec<T>::two(v[0], v[1]);
    } else {
#pragma unroll
        for (int j = 0; j < V; j += 4)
            *reinterpret_cast<typename GroupVec<T>::four*>(p + j) = typename GroupVec<T>::four(v[j], v[j + 1], v[j + 2], v[j + 3]);
    }
}

// integer labels as a plane of T: float through store_group, int64_t as 16-byte pairs
template <class T, int V>
__device__ __forceinline__ void store_group_as(T* p, const int (&v)[V]) {
    if constexpr (std::is_same_v<T, int64_t>) {
        static_assert(V == 1 || V % 2 == 0, "int64 labels go out one by one or in pairs");
        if constexpr (V == 1) *p = v[0];
        else
#pragma unroll
            for (int j = 0; j < V; j += 2) *reinterpret_cast<longlong2*>(p + j) = make_longlong2(v[j], v[j + 1]);
    } else {
        T t[V];
#pragma unroll
        for (int j = 0; j < V; ++j) t[j] = (T)v[j];
        store_group(p, t);
    }
}

// V label bytes as ONE word of V bytes (V = 16: one 16-byte store), byte j = v[j], p on the V-byte grid.  A uint8_t plane takes values its
// launcher has bounded to 0 .. 255 as they are; an int8_t plane takes the low byte (-1 is a value there).
template <class B, int V>
__device__ __forceinline__ void store_bytes(B* p, const int (&v)[V]) {
    static_assert(sizeof(B) == 1 && (V == 1 || V == 2 || V == 4 || V == 16), "1, 2, 4 or 16 bytes");
    if constexpr (V == 1) {
        *p = (B)v[0];
    } else {
        constexpr int N = V < 4 ? V : 4;              // bytes per word
        uint32_t w[V / N];
#pragma unroll
        for (int q = 0; q < V / N; ++q) {
            w[q] = 0;
#pragma unroll
            for (int j = 0; j < N; ++j) w[q] |= (std::is_signed_v<B> ? (uint32_t)(uint8_t)v[N * q + j] : (uint32_t)v[N * q + j]) << (8 * j);
        }
        if constexpr (V == 2) *reinterpret_cast<uint16_t*>(p) = (uint16_t)w[0];
        else store_group(reinterpret_cast<uint32_t*>(p), w);
    }
}

// ---------------------------------------------------------------- host half
// the per-file switch that forces the V = 1 kernels (the tests compare them with the vector ones bit for bit); read at every call
inline bool scalar_forced(const char* env) { return getenv(env) != nullptr; }

// every NON-NULL pointer is a multiple of `bytes` (a power of two): the grid a lane's access of that size needs
template <class... P>
inline bool on_grid(size_t bytes, const P*... p) {
    assert(bytes && (bytes & (bytes - 1)) == 0);
    return ((... | (uintptr_t)p) & (bytes - 1)) == 0;
}

// every extent or element stride is a multiple of v: a group never crosses a row, plane or channel it must not cross
template <class... N>
inline bool multiples_of(int v, N... n) { return (... && (n % v == 0)); }

// grid.x for n elements at V per lane, 256 lanes per workgroup (the last group may be partial where the kernel allows it)
inline unsigned lane_blocks(long n, int V) { return (unsigned)(((n + V - 1) / V + 255) / 256); }

// f(std::integral_constant<int, v>) for the v of Vs... that equals V: `dispatch_lanes<4, 1>(V, [&](auto v) { launch kernel<decltype(v)::value> })`.
// Any small set of integers that name a template argument will do (seg_epilogue picks its channel bound this way too); a V that is
// none of Vs is the caller's mistake: nothing would be launched, hence the assert.
template <int... Vs, class F>
inline void dispatch_lanes(int V, F f) {
    const bool ran = (... || (V == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false));
    assert(ran);
    (void)ran;
}

}  // namespace ivosw
