// qhuff_tabs_impl.h -- a set of dynamic tables and a table per section
// (struct qhuff_dyn_tables, include/qhuff.h): what a section's walk and a
// header's lookup read of their table, and the host forms' checks.
//
// The same source runs as device code (qhuff_hdrscan_tabs.hip,
// qhuff_lookup_tabs.hip: a lane forms the view of its section's table) and as
// plain C++ on the host (the _cpu forms, qhuff_frames.cpp).  The rules are
// not here: the walk is qhuff_scan_impl.h's with the DynWin its dyn_win_tabs
// forms (the view of a section's table, TabView, is defined there), the
// lookup qhuff_lookup_dyn_impl.h's with the window translated to ordinals.
#pragma once
#include <stdint.h>

#include "../../include/qhuff.h"
#include "qhuff_lookup_dyn_impl.h"
#include "qhuff_scan_impl.h"

namespace qhuff {

using scan::TabView;
using scan::tab_view;

// the table that holds entry k < D: the last c with ent[c] <= k (ent values
// clamped to D; within [0, T - 1] and after at most 32 steps whatever ent
// holds).  T != 0.
template <class P>
QH_HDI uint32_t
tab_of_entry(P ent, uint32_t T, uint32_t D, uint32_t k)
{
    uint32_t lo = 0, hi = T - 1;
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        const uint32_t e = ent[mid];
        if ((e < D ? e : D) <= k)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// What is mixed into an entry's first slot for its table: a bijection of c
// whose low bits depend on all of c's (tab_mix(0) = 0: one table is the
// _dyn index).
QH_HDI constexpr uint32_t
tab_mix(uint32_t c)
{
    uint32_t x = c * 0x9E3779B1u;
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    return x;
}

// A section as the lookup sees it: its window as global ordinals [glo, ghi)
// (inside its table's, so the probe's filter rejects other tables' entries by
// ordinal alone), delta = first - e0 (ordinal + delta = the table's absolute
// index, modulo 2^32), its Base (absolute) and its table's slot mix and
// max_entries.
struct TabSection
{
    uint32_t glo, ghi, delta, mix, base, max_entries;
};

template <class P>
QH_HDI TabSection
tab_section(P ent, P first, P max_entries, uint32_t T, uint32_t D, P sec_tab,
            P sec_win, P sec_base, uint64_t s)
{
    const TabView v = tab_view(ent, first, max_entries, T, D, sec_tab, s);
    const uint64_t lo = sec_win ? sec_win[2 * s] : v.first;
    const uint64_t hi = sec_win ? sec_win[2 * s + 1] : (uint64_t) v.first + v.d;
    const DynRange w = dyn_window(lo, hi, v.first, v.d, v.max_entries);
    TabSection t;
    t.delta = v.first - v.e0;
    t.glo = w.lo - t.delta;
    t.ghi = w.hi - t.delta;
    t.mix = tab_mix(v.c);
    t.base = sec_base ? dyn_base(sec_base[s], v.first, v.d) : w.hi;
    t.max_entries = v.max_entries;
    return t;
}

// a hit among the entries (a global ordinal) as its table's absolute index
QH_HDI DynHit
tab_hit(DynHit h, uint32_t delta)
{
    if (h.dyn != QHUFF_DYN_NONE)
        h.dyn += delta;
    return h;
}

// The host and _cpu forms' check of a set of tables, of m sections' tables,
// windows (sec_win null: each section's whole table) and Bases (or null):
// QHUFF_OK, QHUFF_EINVAL or QHUFF_ERANGE as include/qhuff.h lists them.
// enc: the encode calls' window rule (a window of at most max_entries).
// *D = ent[T]; *longest = the longest name + value of all entries.
inline int
tabs_check(const ::qhuff_dyn_tables *t, const uint32_t *sec_tab,
           const uint32_t *sec_win, const uint32_t *sec_base, uint32_t m,
           bool enc, uint32_t *D, uint32_t *longest)
{
    *D = 0;
    *longest = 0;
    if (!t || (t->T && (!t->ent || !t->first || !t->max_entries
                        || (m && !sec_tab))))
        return QHUFF_EINVAL;
    const uint32_t T = t->T;
    if (T && t->ent[0] != 0)
        return QHUFF_EINVAL;
    for (uint32_t c = 0; c < T; ++c)
        if (t->ent[c + 1] < t->ent[c])
            return QHUFF_EINVAL;
    const uint32_t d_all = T ? t->ent[T] : 0;
    if (d_all > kDynMaxD)
        return QHUFF_ERANGE;
    if (d_all && (!t->off || !t->bytes))
        return QHUFF_EINVAL;
    for (uint32_t c = 0; c < T; ++c)
        if ((uint64_t) t->first[c] + (t->ent[c + 1] - t->ent[c])
                > 0xffffffffull)
            return QHUFF_ERANGE;
    for (uint64_t i = 0; i < 2ull * d_all; ++i)
        if (t->off[i + 1] < t->off[i])
            return QHUFF_EINVAL;
    for (uint64_t k = 0; k < d_all; ++k)
    {
        const uint32_t l = t->off[2 * k + 2] - t->off[2 * k];
        *longest = l > *longest ? l : *longest;
    }
    for (uint64_t s = 0; s < m; ++s)
    {
        if (T && sec_tab[s] >= T)
            return QHUFF_EINVAL;
        const uint32_t c = T ? sec_tab[s] : 0;
        const uint64_t d = T ? t->ent[c + 1] - t->ent[c] : 0;
        const uint64_t t0 = T ? t->first[c] : 0, t1 = t0 + d;
        const uint64_t me = T ? t->max_entries[c] : 0;
        if (sec_win)
        {
            const uint64_t lo = sec_win[2 * s], hi = sec_win[2 * s + 1];
            if (lo < t0 || hi < lo || hi > t1 || (enc && me && hi - lo > me))
                return QHUFF_EINVAL;
        }
        else if (enc && me && d > me)
            return QHUFF_EINVAL;
        if (sec_base && sec_base[s] > t1)
            return QHUFF_EINVAL;
    }
    *D = d_all;
    return QHUFF_OK;
}

}  // namespace qhuff
