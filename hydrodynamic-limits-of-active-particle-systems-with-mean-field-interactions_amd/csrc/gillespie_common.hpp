// gillespie_common.hpp -- host side of what the two shapes of the exact event loop share: gillespie_hip.hip (many systems,
// each in one workgroup's LDS) and gillespie_big_hip.hip (large systems in global memory), behind the C ABI of
// include/gillespie*.h.  One call record (GilIo: what every run function takes; GilExtras: what one of them adds), the
// variant tags of the two kernel families, and one staging path: the helpers below upload the common inputs, allocate and
// fetch the common outputs and the structure / capture / profile / checkpoint extras for all three drivers (batch_run and
// mixed_run of gillespie_hip.hip, gil_large_run of gillespie_big_hip.hip), templated on the driver's argument struct.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "gillespie.h"
#include "aps_common.hpp"
#include "dev_mem.hpp"
#include "gillespie_structure.hpp"        // GilsArgs, gils_phase_table
#include "gillespie_capture.hpp"          // GilcCall, GilcArgs
#include "gillespie_profile.hpp"          // GilpCall, GilpArgs
#include "gillespie_resume.hpp"           // GilrCall, GilrArgs

struct gilx_variants;                      // include/gillespie_mixed.h

// what gilxs_run adds to gilx_run: the structure sums (rows optional) and their window reduction
struct GilxsCall { int k_max, first_obs; double *structure_obs, *head_obs, *window; int32_t *n_window, *n_empty; };

// What every run function takes: the start states, the caller's random numbers, the nine common outputs and the kernel time.
// Any output may be null.  A resumable launch reads its start state from GilExtras::rs and leaves n0 .. bound0 null.
struct GilIo {
    const int32_t *n0, *pos0; const int8_t *sigma0; const uint8_t *bound0; const double *uniforms;
    int32_t *pos_obs; int8_t *sigma_obs; uint8_t *flags_obs; int64_t *scalars_obs;
    int32_t *n_recorded; int64_t *n_events; double *t_final, *exits; int32_t *n_exits; double *kernel_ms;
    bool states() const { return pos_obs || sigma_obs || flags_obs; }
};

// What one entry point adds, at most one of: gils_run's rows (k_max modes, from observation first_obs on), gilc_run's call,
// gilp_run's, the start state of gilr_run / gilrm_run (checked by gilr_prepare; it comes back as the end state), gilxs_run's call,
// gilxm_run's variants (the large shape's mixed launch).  The resumable mixed launches (include/gillespie_mixed_resume.h) have
// `rs` (checked by gilxr_prepare) next to `xs` or `mx`; gilxp_run (include/gillespie_mixed_profile.h) has `prof` in a mixed launch
// (large shape: next to `mx`).  The resumable profile launches (include/gillespie_profile_resume.h) have `prof` next to `rs`, the
// mixed one in a mixed launch; prof->first_obs then counts within the segment's slice.
struct GilExtras {
    int k_max = 0, first_obs = 0; double *structure_obs = nullptr;
    const GilcCall *cap = nullptr; const GilpCall *prof = nullptr; GilrCall *rs = nullptr; const GilxsCall *xs = nullptr;
    const gilx_variants *mx = nullptr;
};

// One enumerator per kernel variant that exists; a kernel family maps each of its own to an argument struct (GilKernelArgs in
// gillespie_hip.hip, BigKernelArgs in gillespie_big_hip.hip), so a combination nobody wrote cannot be instantiated.
enum class GilKind { Plain, Structure, Capture, Profile, Mixed, MixedStructure, Resume, MixedResume, MixedStructureResume, MixedProfile,
                     ProfileResume, MixedProfileResume };

namespace {

constexpr int64_t GIL_PLAN_MAX_BYTES = 1ll << 38;   // work + output bytes a plan accepts without asking a device

// the rate code's parameters of a run: no time step, no caller's flip table yet (gil_upload_flip_table)
inline Model gil_model(const gil_params *p) {
    Model M{};
    M.L = p->L; M.K = p->K; M.periodic = p->periodic ? 1 : 0; M.field_mode = p->sigma_grid > 0.0 ? 1 : 0;
    M.minus_anchor = p->minus_anchor ? 1 : 0; M.immobilize = p->immobilize ? 1 : 0; M.suppress_flip = p->suppress_flip ? 1 : 0;
    M.crowding = p->crowding ? 1 : 0; M.rate_diffusion = p->rate_diffusion; M.rate_active = p->rate_active;
    M.k_on = p->k_on; M.k_off = p->k_off; M.k_exit = p->k_exit; M.dt = 0.0;
    M.seed_lo = (uint32_t)p->seed; M.seed_hi = (uint32_t)(p->seed >> 32); M.ens_base = 0;
    M.flip_n = 0; M.flip_tab = nullptr;
    return M;
}

// nullptr when the n particles of one initial state are acceptable, else the text of the complaint
inline const char *gil_check_state(const gil_params *p, int n, const int32_t *pos, const int8_t *sigma) {
    std::vector<int> occ((size_t)p->L, 0);
    for (int i = 0; i < n; ++i) {
        if (pos[i] < 0 || pos[i] >= p->L) return "position outside [0, L)";
        if (++occ[(size_t)pos[i]] > p->K) return "site capacity exceeded";
        if (sigma[i] != 1 && sigma[i] != -1) return "sigma must be +1 or -1";
    }
    return nullptr;
}

// nullptr when a caller's flip table is acceptable (or absent), else the text of the complaint: aps_set_flip_table's rules.
// A negative or non-finite rate would make a particle's cumulative sums non-monotone on the device.  Host arithmetic only:
// the drivers ask before they touch the device.
inline const char *gil_check_flip_table(const gil_params *p) {
    if (!p->flip_table) return nullptr;
    if (p->flip_n < 1 || p->flip_n > (1 << 24)) return "flip_n must be in [1, 2^24]";
    for (size_t i = 0, n = (size_t)2 * ((size_t)p->flip_n + 1); i < n; ++i)
        if (!(p->flip_table[i] >= 0.0) || !std::isfinite(p->flip_table[i])) return "rates must be finite and >= 0";
    return nullptr;
}

// a caller's flip_rate_fn, tabulated (aps_set_flip_table's layout): onto the device and into the model
inline int gil_upload_flip_table(OneShot &job, const gil_params *p, Model &M) {
    if (!p->flip_table) return 0;
    if (const char *why = gil_check_flip_table(p)) return job.fail(job.e_arg, std::string(job.who) + ": " + why);
    if (int rc = job.upload(&M.flip_tab, p->flip_table, (size_t)2 * ((size_t)p->flip_n + 1), "flip_table")) return rc;
    M.flip_n = p->flip_n;
    return 0;
}

// empty when every system's start state is acceptable, else the text of the complaint; n0_text: what an n0 outside [0, n_cap]
// is called (nullptr: with the numbers, as the mixed launches word it)
inline std::string gil_check_start(const gil_params *p, const GilIo &io, const char *n0_text) {
    const int ncap = p->n_cap;
    for (int s = 0; s < p->n_systems; ++s) {
        if (io.n0[s] < 0 || io.n0[s] > ncap)
            return n0_text ? n0_text : "n0 = " + std::to_string(io.n0[s]) + " of system " + std::to_string(s) + " is outside [0, n_cap = " + std::to_string(ncap) + "]";
        if (const char *why = gil_check_state(p, io.n0[s], io.pos0 + (size_t)s * ncap, io.sigma0 + (size_t)s * ncap)) return why;
    }
    return "";
}

// the plans' refusal of more than 2^38 bytes: 0, or GIL_ERR_ARG with the text in `err`
inline int gil_refuse_plan_bytes(const char *who, std::string &err, int64_t work, int64_t outb) {
    if (work + outb <= GIL_PLAN_MAX_BYTES) return GIL_OK;
    err = std::string(who) + ": the batch needs " + std::to_string(work) + " bytes of work memory and " + std::to_string(outb) +
          " bytes of outputs, more than the " + std::to_string(GIL_PLAN_MAX_BYTES) + " bytes a plan accepts";
    return GIL_ERR_ARG;
}

// the drivers' refusal of more than the device has free (after select_device)
inline int gil_refuse_device_bytes(OneShot &job, int64_t work, int64_t outb) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return job.fail(job.e_hip, std::string(job.who) + ": hipMemGetInfo failed");
    if ((uint64_t)(work + outb) > (uint64_t)free_b)
        return job.fail(job.e_arg, std::string(job.who) + ": the batch needs " + std::to_string(work) + " bytes of work memory and " +
                                       std::to_string(outb) + " bytes of outputs, the device has " + std::to_string(free_b) + " bytes free");
    return 0;
}

// The inputs every kernel reads and the nine outputs every kernel writes, into the driver's argument struct `a`.  The start
// states are uploaded where io has them (n_start entries of pos0 / sigma0 / bound0); scalar_tables: front_lo and a blocking
// table of n_block bytes, which only the scalar sums read.
template <class Args>
int gil_stage_common(OneShot &job, Args &a, const gil_params *p, const GilIo &io, const std::vector<double> &table, size_t n_start,
                     bool scalar_tables, const uint8_t *block_table, size_t n_block) {
    const size_t S = (size_t)p->n_systems, SN = S * p->n_cap, SO = S * p->n_obs;
    UP(betas, p->beta, S); UP(table, table.data(), table.size()); UP(times, p->times_obs, (size_t)p->n_obs);
    if (io.n0) { UP(n0, io.n0, S); UP(pos0, io.pos0, n_start); UP(sigma0, io.sigma0, n_start); }
    if (io.n0 && io.bound0) UP(bound0, io.bound0, n_start);
    if (p->anchor_mask) UP(anchor, p->anchor_mask, (size_t)p->L);
    if (scalar_tables && p->front_lo) UP(front_lo, p->front_lo, (size_t)p->L);
    if (scalar_tables && block_table) UP(block_table, block_table, n_block);
    if (int rc = gil_upload_flip_table(job, p, a.m)) return rc;
    if (io.uniforms) UP(uniforms, io.uniforms, S * p->max_events * 4);
    OUT(pos_obs, io.pos_obs, SO * p->n_cap); OUT(sigma_obs, io.sigma_obs, SO * p->n_cap); OUT(flags_obs, io.flags_obs, SO * p->n_cap);
    OUT(scalars, io.scalars_obs, SO * GIL_NSCALARS);
    OUT(n_recorded, io.n_recorded, S); OUT(n_events, io.n_events, S); OUT(t_final, io.t_final, S);
    OUT(exits, io.exits, SN * 3); OUT(n_exits, io.n_exits, S);
    return 0;
}

template <class Args>
int gil_fetch_common(OneShot &job, const Args &a, const gil_params *p, const GilIo &io) {
    const size_t S = (size_t)p->n_systems, SN = S * p->n_cap, SO = S * p->n_obs;
    DOWN(io.pos_obs, pos_obs, SO * p->n_cap * 4); DOWN(io.sigma_obs, sigma_obs, SO * p->n_cap); DOWN(io.flags_obs, flags_obs, SO * p->n_cap);
    DOWN(io.scalars_obs, scalars, SO * GIL_NSCALARS * 8);
    DOWN(io.n_recorded, n_recorded, S * 4); DOWN(io.n_events, n_events, S * 8); DOWN(io.t_final, t_final, S * 8);
    DOWN(io.exits, exits, SN * 3 * 8); DOWN(io.n_exits, n_exits, S * 4);
    return 0;
}

// The structure sums: rows (where wanted) and the phase table, which is filled here, before the timed window
template <class Args>
int gil_stage_structure(OneShot &job, Args &a, const gil_params *p, int k_max, int first_obs, bool want_rows, bool phase_in_lds) {
    double *phase = nullptr;
    if (want_rows) if (int rc = job.alloc(&a.st.rows, (size_t)p->n_systems * p->n_obs * (4 + 2 * (size_t)k_max), "structure_obs")) return rc;
    if (int rc = job.alloc(&phase, (size_t)2 * p->L, "phase")) return rc;
    a.st.phase = phase; a.st.k_max = k_max; a.st.first_obs = first_obs; a.st.phase_in_lds = phase_in_lds ? 1 : 0;
    hipLaunchKernelGGL(gils_phase_table, dim3((unsigned)((p->L + 255) / 256)), dim3(256), 0, nullptr, phase, p->L);
    return 0;
}

template <class Args>
int gil_fetch_structure(OneShot &job, const Args &a, const gil_params *p, double *structure_obs) {
    return job.download(structure_obs, a.st.rows, (size_t)p->n_systems * p->n_obs * (4 + 2 * (size_t)a.st.k_max) * 8, "structure_obs");
}

// The capture statistics; tbind_global: the bind times are work memory (large shape; the batch shape keeps them in LDS)
template <class Args>
int gil_stage_capture(OneShot &job, Args &a, const gil_params *p, const GilcCall &c, bool tbind_global) {
    const size_t S = (size_t)p->n_systems, SO = S * p->n_obs;
    a.cp.n_groups = c.n_groups; a.cp.c_bins = c.c_bins; a.cp.h_bins = c.h_bins; a.cp.first_obs = c.first_obs; a.cp.h_dt = c.h_dt;
    if (c.group_of_site) UP(cp.group, c.group_of_site, (size_t)p->L);
    WORK(cp.rows, SO * (size_t)(GILC_FIXED + c.n_groups + c.c_bins));
    WORK(cp.life_hist, S * 2 * c.h_bins); WORK(cp.life_sums, S * 4);
    if (tbind_global) WORK(cp.tbind, S * p->n_cap);
    return 0;
}

template <class Args>
int gil_fetch_capture(OneShot &job, const Args &a, const gil_params *p, const GilcCall &c) {
    const size_t S = (size_t)p->n_systems, SO = S * p->n_obs;
    if (int rc = job.download(c.capture_obs, a.cp.rows, SO * (size_t)(GILC_FIXED + c.n_groups + c.c_bins) * 8, "capture_obs")) return rc;
    if (int rc = job.download(c.life_hist, a.cp.life_hist, S * 2 * c.h_bins * 8, "life_hist")) return rc;
    return job.download(c.life_sums, a.cp.life_sums, S * 4 * 8, "life_sums");
}

// The ensemble profiles
template <class Args>
int gil_stage_profile(OneShot &job, Args &a, const gil_params *p, const GilpCall &c) {
    const size_t S = (size_t)p->n_systems, SO = S * p->n_obs, GO = (size_t)c.n_groups * p->n_obs;
    a.pf.n_bins = c.n_bins; a.pf.width = (p->L + c.n_bins - 1) / c.n_bins; a.pf.n_used = (p->L + a.pf.width - 1) / a.pf.width;
    a.pf.first_obs = c.first_obs; a.pf.want_field = c.want_field;
    if (c.group_of_system) UP(pf.group, c.group_of_system, S); else WORK(pf.group, S);   // zero-filled: group 0
    WORK(pf.sums, GO * GILP_COLS * c.n_bins); WORK(pf.members, GO);
    if (c.profile_obs) WORK(pf.rows, SO * 3 * c.n_bins);
    return 0;
}

template <class Args>
int gil_fetch_profile(OneShot &job, const Args &a, const gil_params *p, const GilpCall &c) {
    const size_t SO = (size_t)p->n_systems * p->n_obs, GO = (size_t)c.n_groups * p->n_obs;
    if (int rc = job.download(c.ensemble_sums, a.pf.sums, GO * GILP_COLS * c.n_bins * 8, "ensemble_sums")) return rc;
    if (int rc = job.download(c.members, a.pf.members, GO * 4, "members")) return rc;
    return job.download(c.profile_obs, a.pf.rows, SO * 3 * c.n_bins * 4, "profile_obs");
}

// The checkpoint a resumable launch starts from.  own_state: the kernel reads the slots' sites from ra.pos and leaves its end
// state in ra.*_out (batch shape; the large shape reads them as pos0 and ends in its global scratch).
inline int gil_stage_checkpoint(OneShot &job, GilrArgs &ra, const gil_params *p, const GilrCall &rs, bool own_state) {
    const size_t S = (size_t)p->n_systems, SN = S * p->n_cap;
    ra.fresh = rs.fresh;
    if (own_state) if (int rc = job.upload(&ra.pos, rs.pos.data(), SN, "checkpoint pos")) return rc;
    if (int rc = job.upload(&ra.ref, rs.ref.data(), SN, "checkpoint ref")) return rc;
    if (int rc = job.upload(&ra.flg, rs.flg.data(), SN, "checkpoint flags")) return rc;
    if (int rc = job.upload(&ra.k_start, rs.k_start.data(), S, "checkpoint next_obs")) return rc;
    if (int rc = job.upload(&ra.t, rs.t.data(), S, "checkpoint t")) return rc;
    if (int rc = job.upload(&ra.n_ev, reinterpret_cast<const long long *>(rs.n_ev.data()), S, "checkpoint n_events")) return rc;
    if (!own_state) return 0;
    if (int rc = job.alloc(&ra.pos_out, SN, "checkpoint pos")) return rc;
    if (int rc = job.alloc(&ra.ref_out, SN, "checkpoint ref")) return rc;
    return job.alloc(&ra.flg_out, SN, "checkpoint flags");
}

// the end state, from wherever the shape left it
inline int gil_fetch_checkpoint(OneShot &job, GilrCall &rs, const gil_params *p, const int32_t *pos, const int32_t *ref, const uint8_t *flg) {
    const size_t SN = (size_t)p->n_systems * p->n_cap;
    if (int rc = job.download(rs.pos.data(), pos, SN * 4, "checkpoint pos")) return rc;
    if (int rc = job.download(rs.ref.data(), ref, SN * 4, "checkpoint ref")) return rc;
    return job.download(rs.flg.data(), flg, SN, "checkpoint flags");
}

}  // namespace

// The entry points of gillespie_hip.hip reach the large-system kernel of gillespie_big_hip.hip through these two: inside the
// library only.  The plan gives the LDS bytes of a workgroup with extra_lds bytes of slots behind the kernel's own, and the
// work bytes of the whole batch; the run is the large-system kernel's driver, gilm_run's, with the extras of the call.
__attribute__((visibility("hidden"))) int gil_large_plan(const char *who, std::string &err, const gil_params *p, int32_t extra_lds,
                                                         int32_t *lds_bytes, int64_t *work_bytes);
__attribute__((visibility("hidden"))) int gil_large_run(const char *who, std::string &err, const gil_params *p, const GilIo &io,
                                                        const GilExtras &ex);
// gil_large_plan for a mixed launch (gilxm_plan's checks and numbers, by host arithmetic): also the longest table's length and the
// doubles of all tables
__attribute__((visibility("hidden"))) int gil_large_mixed_plan(const char *who, std::string &err, const gil_params *p, const gilx_variants *v,
                                                               bool want_states, int32_t extra_lds, int32_t *lds_bytes, int64_t *work_bytes,
                                                               int32_t *max_tlen, int64_t *table_doubles);
