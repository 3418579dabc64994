// gillespie_resume.hpp -- what the resumable instantiations of the two exact-loop kernels share (include/gillespie_resume.h, and
// for mixed batches include/gillespie_mixed_resume.h):
// the start state a launch reads instead of n0 / pos0 / sigma0 / bound0, where it leaves its end state, and the host side
// that checks a checkpoint, makes one of a fresh initial state, and fills the caller's from the launch's outputs.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "gillespie_resume.h"
#include "gillespie_mixed_resume.h"

// Host side: the start state of a launch, checked, and what to do with its end.
struct GilrCall {
    std::vector<int32_t> pos, ref, k_start, next_obs;
    std::vector<uint8_t> flg, skipped;     // skipped: the system had ended before this launch's slice
    std::vector<double> t;
    std::vector<int64_t> n_ev;
    int32_t fresh = 0, obs_first = 0;
    gil_checkpoint *to = nullptr;
    // a mixed launch (include/gillespie_mixed_resume.h, gilxr_prepare) also has every system's slot count and, with the
    // structure sums (k_max > 0), the window accumulators it starts from (null: zero) and where they go at the end
    std::vector<int32_t> n_slots;
    int32_t k_max = 0;
    const gilx_checkpoint *xfrom = nullptr;
    gilx_checkpoint *xto = nullptr;
};

namespace {

// Device side.  Inputs [n_systems][n_cap] and [n_systems]; the flags are the loop's own bits (F_PLUS, F_BOUND, F_ALIVE =
// GILR_PLUS, GILR_BOUND, GILR_ALIVE).  The end time, event count and row reached leave through the loop's t_final, n_events
// and n_recorded.  The large-system kernel keeps its state in global memory: its end state is read from there, *_out unused.
struct GilrArgs {
    const int32_t *pos, *ref, *k_start;    // k_start: the system's first row of this launch's slice
    const uint8_t *flg;
    const double *t;
    const long long *n_ev;
    int32_t *pos_out, *ref_out;
    uint8_t *flg_out;
    int32_t fresh;                         // 1: the start state is an initial condition (row 0 is recorded before the first event)
};

static_assert(GILR_PLUS == 1 && GILR_BOUND == 2 && GILR_ALIVE == 4, "the checkpoint's flag bits are the loop's");

// Fills `c` from the checkpoint `from`, or from the initial state where from == nullptr (the caller has checked that one with
// gil_check_state).  Empty string, or the text of the complaint.
inline std::string gilr_prepare(const gil_params *p, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
                                int32_t obs_first, const gil_checkpoint *from, gil_checkpoint *to, GilrCall &c) {
    const size_t S = (size_t)p->n_systems, N = (size_t)p->n_cap;
    if (obs_first < 0) return "obs_first must not be negative";
    if (to && !(to->pos && to->flags && to->ref && to->t && to->n_events && to->next_obs)) return "null array in the checkpoint `to`";
    c.pos.assign(S * N, 0); c.ref.assign(S * N, -1); c.flg.assign(S * N, 0);
    c.k_start.assign(S, 0); c.next_obs.assign(S, obs_first); c.skipped.assign(S, 0); c.t.assign(S, 0.0); c.n_ev.assign(S, 0);
    c.fresh = from ? 0 : 1; c.obs_first = obs_first; c.to = to;
    if (!from) {
        for (size_t s = 0; s < S; ++s)
            for (size_t i = 0; i < (size_t)n0[s]; ++i) {
                c.pos[s * N + i] = pos0[s * N + i];
                c.flg[s * N + i] = (uint8_t)(GILR_ALIVE | (sigma0[s * N + i] > 0 ? GILR_PLUS : 0) | ((bound0 && bound0[s * N + i]) ? GILR_BOUND : 0));
            }
        return "";
    }
    if (!(from->pos && from->flags && from->ref && from->t && from->n_events && from->next_obs)) return "null array in the checkpoint `from`";
    std::vector<int> occ((size_t)p->L);
    for (size_t s = 0; s < S; ++s) {
        std::fill(occ.begin(), occ.end(), 0);
        for (size_t i = 0; i < N; ++i) {
            const int32_t x = from->pos[s * N + i], r = from->ref[s * N + i];
            const uint8_t f = from->flags[s * N + i];
            if (x < 0 || x >= p->L) return "checkpoint: position outside [0, L)";
            if (r < -1 || r >= p->L) return "checkpoint: displacement origin outside [-1, L)";
            if (f & ~(GILR_PLUS | GILR_BOUND | GILR_ALIVE)) return "checkpoint: unknown flag bits";
            if ((f & GILR_ALIVE) && ++occ[(size_t)x] > p->K) return "checkpoint: site capacity exceeded";
            c.pos[s * N + i] = x; c.ref[s * N + i] = r; c.flg[s * N + i] = f;
        }
        const double t = from->t[s];
        const int64_t ne = from->n_events[s];
        const int32_t no = from->next_obs[s];
        if (!(t >= 0.0)) return "checkpoint: t must be a time >= 0 or +inf";
        if (ne < 0) return "checkpoint: negative event count";
        if (no < 0 || (int64_t)no > (int64_t)obs_first + p->n_obs) return "checkpoint: next_obs lies beyond this launch's observations";
        c.t[s] = t; c.n_ev[s] = ne; c.next_obs[s] = no;
        if (no < obs_first) {
            if (!(t > p->T) && ne < p->max_events) return "checkpoint: next_obs lies before obs_first and the system has not ended";
            c.skipped[s] = 1; c.k_start[s] = p->n_obs;        // no row of this slice is its own
        } else c.k_start[s] = no - obs_first;
    }
    return "";
}

// After the launch: n_recorded of the systems that were skipped, and the caller's checkpoint (pos / flg / ref are the
// downloaded end state).
inline void gilr_finish(const gil_params *p, GilrCall &c, int32_t *n_recorded, const int64_t *n_events, const double *t_final) {
    const size_t S = (size_t)p->n_systems, N = (size_t)p->n_cap;
    for (size_t s = 0; s < S; ++s) if (c.skipped[s]) n_recorded[s] = 0;
    if (!c.to) return;
    for (size_t q = 0; q < S * N; ++q) { c.to->pos[q] = c.pos[q]; c.to->flags[q] = c.flg[q]; c.to->ref[q] = c.ref[q]; }
    for (size_t s = 0; s < S; ++s) {
        c.to->t[s] = t_final[s]; c.to->n_events[s] = n_events[s];
        c.to->next_obs[s] = c.skipped[s] ? c.next_obs[s] : c.obs_first + n_recorded[s];
    }
}

// The same for a mixed launch: gilr_prepare on the checkpoint's base, then what gilx_checkpoint adds -- the slot counts (from
// n0 on a fresh start) and, where k_max > 0 (a structure launch), the window sums.
inline std::string gilxr_prepare(const gil_params *p, int32_t k_max, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0,
                                 const uint8_t *bound0, int32_t obs_first, const gilx_checkpoint *from, gilx_checkpoint *to, GilrCall &c) {
    const size_t S = (size_t)p->n_systems, N = (size_t)p->n_cap;
    if (to && !to->n_slots) return "null n_slots in the checkpoint `to`";
    if (to && k_max > 0 && !(to->window && to->n_window && to->n_empty)) return "null window, n_window or n_empty in the checkpoint `to` with k_max > 0";
    if (from && !from->n_slots) return "null n_slots in the checkpoint `from`";
    if (from && k_max > 0 && !(from->window && from->n_window && from->n_empty)) return "checkpoint: null window, n_window or n_empty with k_max > 0";
    const std::string why = gilr_prepare(p, n0, pos0, sigma0, bound0, obs_first, from ? &from->base : nullptr, to ? &to->base : nullptr, c);
    if (!why.empty()) return why;
    c.k_max = k_max; c.xfrom = from; c.xto = to;
    c.n_slots.assign(S, 0);
    if (!from) { for (size_t s = 0; s < S; ++s) c.n_slots[s] = n0[s]; return ""; }
    for (size_t s = 0; s < S; ++s) {
        const int32_t ns = from->n_slots[s];
        if (ns < 0 || (size_t)ns > N)
            return "checkpoint: n_slots = " + std::to_string(ns) + " of system " + std::to_string(s) + " is outside [0, n_cap = " + std::to_string(N) + "]";
        for (size_t i = (size_t)ns; i < N; ++i)
            if (from->base.flags[s * N + i])
                return "checkpoint: slot " + std::to_string(i) + " of system " + std::to_string(s) + " has flags " + std::to_string((int)from->base.flags[s * N + i]) +
                       " but lies at or beyond n_slots = " + std::to_string(ns);
        c.n_slots[s] = ns;
    }
    if (k_max > 0)
        for (size_t s = 0; s < S; ++s) {
            if (from->n_window[s] < 0) return "checkpoint: negative n_window = " + std::to_string(from->n_window[s]) + " of system " + std::to_string(s);
            if (from->n_empty[s] < 0) return "checkpoint: negative n_empty = " + std::to_string(from->n_empty[s]) + " of system " + std::to_string(s);
        }
    return "";
}

// After a mixed launch: gilr_finish, and the slot counts.  The window sums were downloaded into `to` by the driver.
inline void gilxr_finish(const gil_params *p, GilrCall &c, int32_t *n_recorded, const int64_t *n_events, const double *t_final) {
    gilr_finish(p, c, n_recorded, n_events, t_final);
    if (c.xto) for (size_t s = 0; s < (size_t)p->n_systems; ++s) c.xto->n_slots[s] = c.n_slots[s];
}

}  // namespace
