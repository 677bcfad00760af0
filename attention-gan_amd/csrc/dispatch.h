// Host only: run-time values -> kernel template arguments.  Each picker calls a generic lambda with Int<> / Bool<> tags; the launch
// site nests the pickers around ONE launch statement and prunes the forms the library does not build with `if constexpr`.
// Which storage types and which 16-bit precision modes exist, and which template arguments they stand for, is written down here only.
#pragma once
#include "agan_common.h"

#include <type_traits>

namespace agan {

// a run-time choice handed to a generic lambda as a type: f(Int<N>{}) instantiates the kernel for N
template <int N> using Int = std::integral_constant<int, N>;
template <bool V> using Bool = std::bool_constant<V>;

// f(Int<DT>) for a storage type (AGAN_DT_*): whatever is not a 16-bit type takes the fp32 form (the entry points check the type)
template <class F> void with_dt(int dt, F&& f) {
    if (dt == AGAN_DT_BF16) f(Int<AGAN_DT_BF16>{});
    else if (dt == AGAN_DT_F16) f(Int<AGAN_DT_F16>{});
    else f(Int<AGAN_DT_F32>{});
}
// f(Int<V>) for the V of the list that equals v; false, and no call, when none does
template <int... Vs, class F> bool with_int(int v, F&& f) {
    return ((v == Vs ? (f(Int<Vs>{}), true) : false) || ...);
}
// f(Int<V>) for the first V of the ascending list with v <= V; the last V takes everything above it too
template <int V, int... Vs, class F> void with_tier(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) f(Int<V>{});
    else if (v <= V) f(Int<V>{});
    else with_tier<Vs...>(v, f);
}
template <class F> void with_bool(bool b, F&& f) {
    if (b) f(Bool<true>{});
    else f(Bool<false>{});
}

// THE table of the 16-bit precision modes: f(Int<ET>, Int<NPL>) with the element type (0 = bf16, 1 = fp16) and the number of operand
// planes a product is split into; false, and no call, for anything else (AGAN_PREC_F32 included)
template <class F> bool with_prec16(int prec, F&& f) {
    switch (prec) {
        case AGAN_PREC_BF16: f(Int<0>{}, Int<1>{}); return true;
        case AGAN_PREC_F16: f(Int<1>{}, Int<1>{}); return true;
        case AGAN_PREC_BF16X3: f(Int<0>{}, Int<2>{}); return true;
        case AGAN_PREC_F16X3: f(Int<1>{}, Int<2>{}); return true;
        case AGAN_PREC_BF16X6: f(Int<0>{}, Int<3>{}); return true;
    }
    return false;
}

// lets Kernel be launched with up to `bytes` of dynamic LDS (the default limit is 64 KB); set once per kernel and process (one
// process drives one GPU), so `bytes` is the most any launch of that kernel asks for
template <auto Kernel> void allow_dynamic_lds(int bytes) {
    static const hipError_t once = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    (void)once;
}

}  // namespace agan
