// nk_kind.h -- kernel selection, host side only: which instantiation of the stepping kernels a configuration runs (NkSweepKind),
// the lifter the pickers are built from (nk_lift), and the process-wide allowance for dynamic LDS above 64 KB (nk_allow_lds).
// The pickers themselves stand next to the kernels they name: nk_sweep_kernel / nk_events_kernel / nk_resident_kernel in
// nk_engine.hip, the group sweeps' in nk_group.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <type_traits>

// The template arguments of k_sweep<GEOM, ROUGH, RBF, PID, SPLIT, LREC, FAST, BOX>: geom 1 = ray-casting tables in LDS, 2 = in
// global memory; fast 0, or 1 / 2 = slice subvolumes with 'nearest' / 'linear' temperatures compiled in; box = box store (no
// cached next hit).  k_events reads geom, rough, rbf and pid of it, k_resident box, pid and lrec, k_sweep_group pid, lrec, fast
// and box.
struct NkSweepKind { int geom; bool rough, rbf, pid, split, lrec; int fast; bool box; };
inline bool operator==(const NkSweepKind &a, const NkSweepKind &b) {
    return a.geom == b.geom && a.rough == b.rough && a.rbf == b.rbf && a.pid == b.pid && a.split == b.split && a.lrec == b.lrec &&
           a.fast == b.fast && a.box == b.box;
}

// Which combinations exist.  Rough facets draw random numbers per particle, so they imply ids.  FAST exists only for the plain
// sweep with tables in LDS, BOX only with tables in LDS and no split.  Everything a normalised kind can say is instantiated;
// the pickers name nothing else.
inline NkSweepKind nk_kind_normalise(NkSweepKind k) {
    k.geom = k.geom == 1 ? 1 : 2;
    k.pid = k.pid || k.rough;
    k.fast = (k.fast && k.geom == 1 && !k.rough && !k.rbf && !k.pid && !k.split) ? (k.fast == 1 ? 1 : 2) : 0;
    k.box = k.box && k.geom == 1 && !k.split;
    return k;
}

// nk_lift(f, a, b, ...) calls f(A, B, ...) with every runtime bool as a std::true_type / std::false_type, so f can use them as
// template arguments (A.value) and prune with `if constexpr`: a combination it does not name is never instantiated.  f states
// its return type (the kernel family's pointer type); an int with two values goes in as a bool (geom == 1, fast == 1).
template <class F>
auto nk_lift(F f) { return f(); }
template <class F, class... Bs>
auto nk_lift(F f, bool b, Bs... rest) {
    auto with = [&](auto B) { return nk_lift([&](auto... cs) { return f(B, cs...); }, rest...); };
    return b ? with(std::true_type{}) : with(std::false_type{});
}

// A launch may ask for more than 64 KB of dynamic LDS only after hipFuncSetAttribute allowed it, and that allowance belongs to
// the kernel FUNCTION for the whole process, not to a context or a grid: nk_allow_lds keeps one high-water mark per (device,
// function) under a mutex and only ever raises it, so two contexts with different needs cannot lower each other's.  Nothing is
// called for bytes <= 64 KB or bytes <= the mark.  Defined once, in nk_engine.hip.
hipError_t nk_allow_lds(const void *fn, size_t bytes);
