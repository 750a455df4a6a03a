// Graph Levenberg-Marquardt engine for MI355X: the numerical core behind
//   a2 CameraPoseAndDeformationOptimization (reference g2o_optimization.cc:148-557) and
//   a3 LocalDeformableBundleAdjustment       (reference g2o_optimization.cc:880-1161),
// i.e. the g2o machinery those functions drive (third_party/g2o/g2o/core/
// optimization_algorithm_levenberg.cpp:57-174, block_solver.hpp:495-562,
// base_fixed_sized_edge.hpp:49-133, robust_kernel_impl.cpp:60-74, sparse_optimizer.cpp:203-285).
//
// Design (MI355X-first, not a translation of g2o's pointer graph):
//   * unknowns: K pose blocks (6) then one 3-dof block per landmark ROW.  Rows are laid out
//     pose-major and every pose's rows are padded to a multiple of ROW_ALIGN, so a workgroup
//     never straddles two poses and the per-pose reductions are plain block reductions.  Inside
//     a pose the rows follow a Morton curve of the initial positions: graph neighbours share
//     cache lines.
//   * every edge is owned by the rows it touches ("incidence lists", sliced-ELL layout: a wave64
//     serves 64/T rows with T lanes per row; element (row r, lane t, step j) of a slice lives at
//     base + j*64 + r*T + t so all loads of a wave are one contiguous 64-element run).  Nothing
//     is scattered: no atomics, no assembly maps, bit-reproducible sums.
//   * H is never assembled, not even block-wise.  (H + lambda I) x = b is solved by preconditioned
//     conjugate gradients (single-reduction Chronopoulos-Gear form) whose operator is applied in
//     FACTORED form from 16-byte incidence records and the LDS-staged linearisation point:
//         spring  : block = qc v v^T, v = x_i - x_j re-formed from staged positions; stores qc  (8 B)
//         damper  : all 16 blocks are +-s I3; stores s                                          (8 B)
//         reproj  : J^T w J with J rebuilt from the fp32 projection Jacobian kept per row       (32 B)
//     A tile (256/T rows) and the rows its incidences reach (the halo) are staged into LDS once per
//     launch; neighbour ids in the records are tile-local.  Large problems: two launches per
//     iteration (k_spmv_f + k_pcg_update).  Small problems (< 32768 rows): ONE launch per iteration
//     (k_pcg_fused: vector update of iteration k-1 + operator of iteration k, halo rows re-derived
//     locally), with, for single-pose problems, a two-level preconditioner whose coarse solve is
//     applied inside that launch (k_coarse_tile / k_coarse_reduce / k_coarse_invert).
//     The reference factorises the same matrix with a sparse Cholesky (no Schur: H_ll is not
//     block diagonal); PCG to 1e-10 relative residual reproduces its iterates.
//   * g2o levels / fixed vertices are byte masks: inactive edges store zero factors, fixed rows
//     are identity rows whose columns vanish because their PCG vectors stay zero.
//   * LM control flow (lambda schedule, accept/reject, <=10 trials) runs on the host exactly as in
//     g2o.  A trial's first PCG batch, the state update and the chi2 evaluation go out in one
//     enqueue and are read back with one synchronisation (results are written by the last kernel
//     into mapped host memory); trials that are going to be rejected are recognised at the 1e-1 ..
//     1e-4 milestones of the inner solve and not solved further (nrs_options.exact_trials = 1
//     turns that off); the iterates are the reference's either way.
//   * XCD-aware launch order: logical tile = (blockIdx % 8) * ceil(nb/8) + blockIdx / 8, so each
//     XCD's L2 serves one contiguous run of rows (neighbour gathers stay inside it).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <new>
#include <system_error>
#include <thread>
#include "nrs_engine.hpp"

#include "nrs_engine_types.hpp"
#include "nrs_engine_linearize.hpp"
#include "nrs_engine_coarse.hpp"
#include "nrs_engine_pcg.hpp"
#include "nrs_engine_skin.hpp"
#include "nrs_engine_nd.hpp"
#include "nrs_engine_kft.hpp"
#include "nrs_engine_plan.hpp"        // the decisions the host packer (setup) and the device packer (devpack) share, and the arena
#include "nrs_engine_setup.hpp"
#include "nrs_engine_kft_setup.hpp"
#include "nrs_devpack_kernels.hpp"     // the device packer: its kernels, ...
#include "nrs_engine_winedges.hpp"     // ... the window-edge construction (WinDev, WinLists: embwin walks the same lists), ...
#include "nrs_engine_devpack.hpp"      // ... and the staged build (DeviceBuild) engine_create runs
#include "nrs_engine_embwin.hpp"
#include "nrs_engine_launch.hpp"      // kernel-variant dispatch (with_lanes, the launchers, Timer) and, through it, nrs_engine_probes.hpp

namespace nrs {

// errors (+ linearisation) at a given state; leaves chi2 (and max diag) in scal[]
template <bool LIN>
static int evaluate(nrs_ctx* c, Engine* e, int which, bool reproj_done = false) {
    if (LIN) { e->d.lin_pose = e->d.pose[which]; e->d.lin_xl = e->d.xl[which]; }   // the PCG kernels re-form factors from it
    const Dev& d = e->d;
    const dim3 gg(((d.sh_ng + 7) / 8) * 8), b(BLK);
    NRS_PROBE(NRS_TRY(lin_clocks_once<LIN>(c, d, d.xl[which]));)
    if (LIN) {
        // LDS path: one fused pass (reprojection + springs + dampers per row); gather path: two
        const int reps = c->opt.profile ? PROFILE_REPS : 1;
        Timer t(c, &c->prof.linearize_ms, &c->prof.linearize_launches, reps);
        for (int r = 0; r < reps; ++r) {
            if (!d.use_lds) hipLaunchKernelGGL((k_reproj<LIN>), gg, b, 0, c->stream, d, d.pose[which], d.xl[which]);
            NRS_TRY(launch_reg<LIN>(c, d, d.xl[which]));
        }
    } else {
        if (!reproj_done) hipLaunchKernelGGL((k_reproj<LIN>), gg, b, 0, c->stream, d, d.pose[which], d.xl[which]);
        if (d.ec_on) hipLaunchKernelGGL(k_chi_edges, dim3(std::max(1, d.ec_nblk)), b, 0, c->stream, d, d.xl[which]);
        else NRS_TRY(launch_reg<LIN>(c, d, d.xl[which]));
    }
    if (LIN) hipLaunchKernelGGL(k_pose_sums, dim3(d.sh_nk), b, 0, c->stream, d);
    if (LIN && d.coarse && !(e->nd && e->nd->on)) {                // (the coarse level is the PCG's: a directly solved engine never reads it -- 50 us per linearisation at 4.4k points)
        const size_t rows = (size_t)(d.tile_rows + d.max_halo), shm = sizeof(double) * 3 * rows + 3 * (rows + 8) + 16;
        NRS_TRY(with_lanes(c, d.T, [&](auto L) { hipLaunchKernelGGL((k_coarse_tile<decltype(L)::value>), dim3(d.n_regblk), b, shm, c->stream, d); }));
        hipLaunchKernelGGL(k_coarse_reduce, dim3(1), b, 0, c->stream, d);
    }
    if (d.sk_n > 0) hipLaunchKernelGGL((k_skin<LIN>), dim3(d.sk_nblk), b, 0, c->stream, d, d.pose[which], d.xl[which]);   // embedded mode: the skinned observations
    if (LIN && d.sk_pcg) {                                         // embedded BA window: their blocks join D / b_l / H_pp / b_p (the PCG path reads those)
        if (d.D_op) NRS_HIP(c, hipMemcpyAsync(d.D_op, d.D, sizeof(double) * 6 * (size_t)d.n_rows, hipMemcpyDeviceToDevice, c->stream));   // (gather path: the operator's copy)
        if (d.sk_nrl > 0) hipLaunchKernelGGL(k_skin_rows, dim3((d.sk_nrl + SK_RPB - 1) / SK_RPB), b, 0, c->stream, d);   // (a rank may hold none)
        hipLaunchKernelGGL(k_skin_pose, dim3((27 * d.sh_nk + BLK - 1) / BLK), b, 0, c->stream, d);   // (own poses)
    }
    if (LIN && e->nd && e->nd->on) {                               // the direct solver's explicit blocks of this linearisation
        const NdVals& nv = e->nd->slot->vals;
        if (nv.ske_ptr) hipLaunchKernelGGL(k_nd_values<true>, dim3((nv.n_ent * ND_SKL + 255) / 256), dim3(256), 0, c->stream, d, nv);
        else hipLaunchKernelGGL(k_nd_values<false>, dim3((nv.n_ent + 255) / 256), dim3(256), 0, c->stream, d, nv);
    }
    if (d.sh_on) {
        // local sums -> packet -> all-reduce over the ranks (pose blocks of the normal equations, chi2,
        // scale, one max-diagonal slot per rank) -> every rank publishes the same scalars
        hipLaunchKernelGGL((k_finalize_pack<LIN>), dim3(1), b, 0, c->stream, d);
        NRS_HIP(c, hipGetLastError());
        NRS_TRY(c->comm->allreduce(c, d.pk_loc, d.pk, (size_t)(2 + d.sh_world + (LIN ? 27 * d.K : 0))));
        hipLaunchKernelGGL((k_finalize_unpack<LIN>), dim3(1), b, 0, c->stream, d, ++c->seq);
    } else {
        // the status words it leaves behind (publish_flags): a directly solved engine's are cleared every time; a re-arming PCG
        // window's by the linearisation (the shadow sets' with them) and by the evaluation that finds the trial's solve finished
        FlagSets fs{};
        int zero = (e->nd && e->nd->on) ? 1 : 0;
        if (e->rearm) {
            zero = LIN ? 1 : 2;
            if (LIN) {
                for (int j = 0; j < e->n_spec; ++j) fs.p[fs.n++] = e->spec[j].flags;
                for (bool& f : e->flags_clean) f = true;
            }
        }
        hipLaunchKernelGGL((k_finalize<LIN>), dim3(1), b, 0, c->stream, d, ++c->seq, zero, fs);
    }
    NRS_HIP(c, hipGetLastError());
    return NRS_OK;
}

// Wait for publication `seq` in the flag block `flags` (mapped host memory: the engine's mirrors, or a shadow set's), enqueued on
// stream st by k_finalize / k_publish / the last PCG launch of a batch -- always the last kernel enqueued there before this.  The
// host polls the sequence word; if it does not show up within ~2 s the stream is synchronised instead, which also surfaces a device
// fault as an error.
static int wait_published(nrs_ctx* c, const int* flags, int seq, hipStream_t st) {
    const volatile int* w = flags + 7;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spins = 0; *w != seq; ++spins) {
        if (spins > 200000) std::this_thread::yield();             // long kernels (large windows): stop hogging the core
        if ((spins & 0xFFFF) == 0xFFFF && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            NRS_HIP(c, hipStreamSynchronize(st));
            if (*w != seq) return c->fail(NRS_ERR_HIP, "device results were not published");
            break;
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return NRS_OK;
}

// One LM trial of a directly solved single-pose engine, enqueued whole: factorise (H + lam I), solve, trial state, chi2, publication
// (sequence number in *seq).  set < 0: on the engine's own arrays and the context's stream -- the launches engine_optimize issues for
// one trial at a time.  set >= 0: the SAME launches on shadow set `set` (nrs_engine_types.hpp SpecSet, nd_alt_dev) and its stream,
// behind the fork event the caller recorded; everything a trial writes is the set's own, everything it reads -- the linearisation, the
// current state -- is shared and read-only while trials are in flight.  Leaves the set's join event recorded behind the publication.
static int direct_trial_enqueue(nrs_ctx* c, Engine* e, int set, double lam, int* seq, int* solve_id, bool in_batch) {   // in_batch: further trials share the device: back passes in turn
    Dev& d = e->d;
    const int cur = e->cur, trial = 1 - e->cur;
    const dim3 g(((d.sh_ng + 7) / 8) * 8), b(BLK);
    if (set < 0) {
        NRS_TRY(nd_solve_enqueue(c, e->nd->S(), lam, nullptr, solve_id, nullptr, in_batch ? c->spec_back[0].get() : nullptr));
        hipLaunchKernelGGL(k_apply_reproj, g, b, 0, c->stream, d, lam, d.pose[cur], d.xl[cur], d.pose[trial], d.xl[trial]);
        NRS_TRY(evaluate<false>(c, e, trial, true));
        *seq = c->seq;
        return NRS_OK;
    }
    const SpecSet& q = e->spec[set];
    struct Restore {                                               // the engine's view and the context's stream come back on every path
        nrs_ctx* c; Engine* e; Dev saved; hipStream_t main;
        ~Restore() { e->d = saved; c->stream = main; }
    } restore{c, e, d, c->stream};
    d.xv = q.xv; d.xp = q.xp; d.part_apply = q.part_apply; d.part_rchi = q.part_rchi; d.part_reg = q.part_reg; d.scal = q.scal; d.flags = q.flags;
    d.h_scal = q.h_scal; d.h_flags = q.h_flags;
    if (d.sk_n > 0) { d.sk_part = q.sk_part; d.sk_chi = q.sk_chi; }
    d.pose[trial] = q.pose; d.xl[trial] = q.xl;
    c->stream = c->spec_stream[set].get();
    NRS_HIP(c, hipStreamWaitEvent(c->stream, c->spec_fork.get(), 0));
    NdDev nd = nd_alt_dev(e->nd->S(), set);
    nd.out_rows = q.xv; nd.out_pose = q.xp; nd.flags = q.flags; nd.abort = q.abort;
    NRS_TRY(nd_solve_enqueue(c, e->nd->S(), lam, &nd, solve_id, c->spec_back[set].get(), c->spec_back[set + 1].get()));
    hipLaunchKernelGGL(k_apply_reproj, g, b, 0, c->stream, d, lam, d.pose[cur], d.xl[cur], q.pose, q.xl);
    NRS_TRY(evaluate<false>(c, e, trial, true));
    *seq = c->seq;
    NRS_HIP(c, hipEventRecord(c->spec_join[set].get(), c->stream));
    return NRS_OK;
}

// The engine seen through shadow set `set` of a PCG BA window (nrs_engine_types.hpp SpecSet; set < 0: the engine itself): everything
// an LM trial writes -- solve vectors, preconditioner inverses, partials, scalars, status words, trial state, host mirrors -- is the
// set's, its launches go to the set's stream, its launches become no-ops once the set's abort word has reached abort_id.  The
// linearisation and the current state are the engine's.  pcg_begin / pcg_enqueue_batch / pcg_advance / evaluate and the host waits
// run unchanged on this view; the engine's own arrays, stream and mirrors come back when it goes.
struct PcgSetView {
    nrs_ctx* c; Engine* e; Dev saved; hipStream_t main; double* hs; int* hf; bool on;
    PcgSetView(nrs_ctx* c_, Engine* e_, int set, int abort_id)
        : c(c_), e(e_), saved(e_->d), main(c_->stream), hs(e_->h_scal), hf(e_->h_flags), on(set >= 0) {
        if (!on) return;
        const SpecSet& q = e->spec[set];
        Dev& d = e->d;
        d.xv = q.xv; d.rv = q.rv; d.uv3 = q.uv3; d.pv = q.pv; d.sv = q.sv; d.wv = q.wv; d.Dinv = q.Dinv; d.Hppinv = q.Hppinv;
        d.xp = q.xp; d.rp = q.rp; d.rp2 = q.rp2; d.up = q.up; d.up2 = q.up2; d.pp = q.pp; d.sp = q.sp;
        d.part_spmv = q.part_spmv; d.part_ru = q.part_ru; d.red = q.red; d.part_ec = q.part_ec;
        d.part_apply = q.part_apply; d.part_rchi = q.part_rchi; d.part_reg = q.part_reg; d.scal = q.scal; d.flags = q.flags;
        d.h_scal = q.h_scal; d.h_flags = q.h_flags;
        d.pose[1 - e->cur] = q.pose; d.xl[1 - e->cur] = q.xl;
        d.abort = q.abort; d.abort_id = abort_id;
        e->h_scal = q.h_scal; e->h_flags = q.h_flags;
        e->view_set = set;
        c->stream = c->spec_stream[set].get();
    }
    ~PcgSetView() { if (on) { e->d = saved; c->stream = main; e->h_scal = hs; e->h_flags = hf; e->view_set = -1; } }
    PcgSetView(const PcgSetView&) = delete;
    PcgSetView& operator=(const PcgSetView&) = delete;
};

// (H + lam I) x = b by block-Jacobi PCG, resumable: pcg_begin, then pcg_advance until it reports
// convergence; with stop_at_peek it also returns as soon as the 1e-4 milestone flag is up.
constexpr double PEEK_RTOL = 1e-1;      // inner-solve accuracy at which a trial is first evaluated
// Gain ratio below which a trial is rejected at the looks taken when the inner solve reaches 1e-2,
// 1e-3, 1e-4 (acceptance needs rho > 0).  The gain ratio of the partially converged step is within
// ~1e-2 / 4e-3 / 2e-3 of the final one at those milestones (second order in the PCG error; measured
// on the a2 and BA problems, profiles/README.md), so the thresholds keep a >10x margin.
constexpr int PEEK_LEVELS = 4;
constexpr double PEEK_MIN_REL_INCREASE = 1e-5;
constexpr double PEEK_RHO_LVL[5] = {0, -1.0, -0.25, -0.1, -0.03};

static int pcg_begin(nrs_ctx* c, Engine* e, double lam, int* it) {
    const Dev& d = e->d;
    // the status words start at zero: left so by the evaluation that published them last (Engine::rearm), or filled here -- after an
    // upload, a trial rejected at a peek or discarded, a solve that ran out of iterations, and on every other kind of engine
    bool& clean = e->flags_clean[1 + e->view_set];
    if (!(e->rearm && clean)) NRS_HIP(c, hipMemsetAsync(d.flags, 0, sizeof(int) * 8, c->stream));
    clean = false;
    if (d.coarse) hipLaunchKernelGGL(k_coarse_invert, dim3(1), dim3(BLK), sizeof(double) * (size_t)d.co_n * d.co_n, c->stream, d, lam);
    hipLaunchKernelGGL(k_trial_setup, dim3(d.sh_nvb), dim3(BLK), 0, c->stream, d, lam);
    if (e->kft && e->kft->on) {                                    // embedded BA window: factorise H + lambda I by keyframe blocks, u_0 = M^-1 b
        NRS_TRY(kft_factor(c, e, e->kft, lam));
        NRS_TRY(kft_apply(c, e->kft, d.rv, d.rp, d.uv3, d.up, d.flags));
        e->kft->apply_pending = false;
    }
    *it = 0;
    return NRS_OK;
}

// enqueue one batch of PCG iterations (no host synchronisation)
// pub_seq != 0: the last launch of the batch publishes the flags under that sequence number (the host waits for it)
static int pcg_enqueue_batch(nrs_ctx* c, Engine* e, double lam, int* it_io, int count = 0, int pub_seq = 0) {
    const Dev& d = e->d;
    const int n_poseblk = (d.K + 3) / 4;
    const double tol2 = c->opt.pcg_rtol * c->opt.pcg_rtol;
    int it = *it_io;
    // profiling contexts poll after every iteration, so that no launch queued behind a converged solve is timed
    int stop = std::min(it + (c->opt.profile ? 1 : count > 0 ? count : c->opt.pcg_batch), c->opt.pcg_max_iters);
    // keyframe-block factorisation: the first step's residual is tested on its own before M^-1 is applied again (k_kft_rnorm,
    // nrs_engine_kft.hpp): the batch that holds iteration 0 ends with it, and u = M^-1 r is enqueued only when the solve goes on
    const bool kft_on = e->kft && e->kft->on;
    const bool kft_lazy = kft_on && it == 0 && stop > 0 && !c->opt.profile && !c->dbg.is_set(SW_KFT_NO_RESIDUAL_TEST);
    if (kft_lazy) stop = 1;
    if (kft_on && e->kft->apply_pending) {
        NRS_TRY(kft_apply(c, e->kft, d.rv, ((it - 1) & 1) ? d.rp : d.rp2, d.uv3, ((it - 1) & 1) ? d.up : d.up2, d.flags));
        e->kft->apply_pending = false;
    }
    for (; it < stop; ++it) {
        const int pub = it + 1 == stop && !kft_lazy ? pub_seq : 0;     // (kft_lazy: k_kft_rnorm is the batch's last launch and publishes)
        NRS_PROBE(if (pcg_clocks_once(c, d, lam, it, tol2, PEEK_RTOL * PEEK_RTOL, pub)) continue;)
        if (d.fused) {
            // frames of <= 32 tiles: every tile on a workgroup of ONE XCD (workgroups are dealt to the XCDs round-robin; the other seven
            // of every eight return at once) -- the vectors then stay in one L2 instead of being written through eight: 19.0 -> 18.0 us
            // per iteration all-in at 543 points, 22.8 -> 21.9 at 1013.  Placement only: the result does not depend on where a workgroup lands.
            const bool one_xcd_off = c->dbg.is_set(SW_NO_ONE_XCD);
            const bool one_xcd = !one_xcd_off && d.n_regblk <= 32;
            Dev d1 = d;
            d1.one_xcd = one_xcd ? 1 : 0;
            const Dev& d = d1;
            const dim3 g(one_xcd ? 8 * d.n_regblk : ((d.n_regblk + 7) / 8) * 8), bb(BLK);
            const size_t shm = sizeof(double) * (6 * (size_t)(d.tile_rows + d.max_halo) + (d.coarse ? 12 * (size_t)d.n_regblk + 16 * CO_MAX : 0));
            if (c->dbg.is_set(SW_CHECK_FUSED) && !d.coarse && d.T == 8) { NRS_TRY(check_fused_launch(c, d, g, shm, lam, it, tol2, PEEK_RTOL * PEEK_RTOL, pub)); continue; }
            NRS_TRY(with_lanes(c, d.T, [&](auto L) {
                constexpr int T = decltype(L)::value;
                hipLaunchKernelGGL((d.coarse ? k_pcg_fused<T, true> : k_pcg_fused<T, false>), g, bb, shm, c->stream, d, lam, it, tol2, PEEK_RTOL * PEEK_RTOL, pub);
            }));
            continue;
        }
        bool skin_op_done = false;                                 // (k_skin_op's workgroups went with the operator's launch)
        bool skin_rows_fused = false;                              // (... and the row pass goes with the vector update's)
        if (d.sh_on && d.sh_world > 1) {
            // sharded: the operator reads u of the neighbouring ranks' boundary keyframes (dampers).  The rows
            // travel on the second stream while the interior tiles run; the boundary tiles follow them.
            NRS_HIP(c, hipEventRecord(c->ev_vec.get(), c->stream));
            NRS_HIP(c, hipStreamWaitEvent(c->comm_stream.get(), c->ev_vec.get(), 0));
            NRS_TRY(c->comm->exchange(c, d.uv3, e->halo, c->comm_stream.get()));
            NRS_HIP(c, hipEventRecord(c->ev_halo.get(), c->comm_stream.get()));
            Dev di = d, db = d;
            for (int cls = 0; cls < 2; ++cls) {
                di.sh_t0[cls] = d.sh_t0[cls] + d.sh_front[cls];
                di.sh_nt[cls] = d.sh_nt[cls] - d.sh_front[cls] - d.sh_back[cls];
                db.sh_nt[cls] = d.sh_front[cls];
                db.sh_t0b[cls] = d.sh_t0[cls] + d.sh_nt[cls] - d.sh_back[cls];
                db.sh_ntb[cls] = d.sh_back[cls];
            }
            // embedded window: the skinned observations reach rows of their own keyframe only -- k_skin_op goes with the interior tiles
            NRS_TRY(launch_spmv(c, di, lam, it, tol2, d.sk_pcg != 0, &skin_op_done));
            if (d.sk_pcg && !skin_op_done) {
                hipLaunchKernelGGL(k_skin_op, dim3(d.sk_nblk), dim3(BLK), 0, c->stream, d, it);
                skin_op_done = true;
            }
            NRS_HIP(c, hipStreamWaitEvent(c->stream, c->ev_halo.get(), 0));
            NRS_TRY(launch_spmv(c, db, lam, it, tol2));
        } else {
            const int reps = c->opt.profile ? PROFILE_REPS : 1;    // (a profiling context has no convergence look-ahead: the launch is idempotent)
            Timer t(c, &c->prof.spmv_ms, &c->prof.spmv_launches, reps);
            if (d.hier && d.ecd) hipLaunchKernelGGL(k_reduce_ru, dim3(1), dim3(BLK), 0, c->stream, d, it);
            for (int r = 0; r < reps; ++r) NRS_TRY(launch_spmv(c, d, lam, it, tol2, d.sk_pcg != 0, &skin_op_done));
        }
        if (d.sk_pcg) {                                            // embedded BA window: H u of the skinned observations' blocks (nrs_engine_skin.hpp)
            if (!skin_op_done) hipLaunchKernelGGL(k_skin_op, dim3(d.sk_nblk), dim3(BLK), 0, c->stream, d, it);
            // the row pass: inside k_pcg_update<true> (for the rows it updates) unless the update is the generic kernel's (a sharded
            // window reduces hierarchically, k_reduce_partials + all-reduce, and still takes the fused form: the update reads red)
            skin_rows_fused = (d.sh_on || !d.hier) && !d.ecd && !c->dbg.is_set(SW_SKIN_ROWS_OWN_LAUNCH);
            if (!skin_rows_fused) hipLaunchKernelGGL(k_skin_op_rows, dim3(d.sh_nvb * BLK / SK_RPB), dim3(BLK), 0, c->stream, d);
        }
        if (d.sh_on) {
            // this rank's dot products and pose sums (other ranks' slots are zero), then the sum over the
            // ranks: every rank continues with the same scalars and updates every pose identically
            Dev dl = d;
            dl.red = d.red_loc;
            hipLaunchKernelGGL(k_reduce_partials, dim3(1 + d.K), dim3(BLK), 0, c->stream, dl);
            NRS_TRY(c->comm->allreduce(c, d.red_loc, d.red, (size_t)(3 + 6 * d.K)));
        } else if (d.hier) hipLaunchKernelGGL(k_reduce_partials, dim3(1 + d.K), dim3(BLK), 0, c->stream, d);
        {
            Timer t(c, &c->prof.vec_ms, &c->prof.vec_launches);
            if (skin_rows_fused) hipLaunchKernelGGL(k_pcg_update<true>, dim3(d.sh_nvb * BLK / SK_RPB + n_poseblk), dim3(BLK), 0, c->stream, d, lam, it, tol2, PEEK_RTOL * PEEK_RTOL, pub);
            else hipLaunchKernelGGL(k_pcg_update<false>, dim3((((d.sh_nvb + 1) / 2 + 7) / 8) * 8 + n_poseblk), dim3(BLK), 0, c->stream,
                                    d, lam, it, tol2, PEEK_RTOL * PEEK_RTOL, pub);
        }
        if (kft_lazy) {
            NRS_TRY(kft_rtest(c, e, e->kft, d.rv, (it & 1) ? d.rp : d.rp2, tol2, pub_seq));
            e->kft->apply_pending = true;
        } else if (kft_on)                                         // u = M^-1 r over the keyframe chains (the update left the block-Jacobi u: overwritten)
            NRS_TRY(kft_apply(c, e->kft, d.rv, (it & 1) ? d.rp : d.rp2, d.uv3, (it & 1) ? d.up : d.up2, d.flags));
    }
    *it_io = it;
    return NRS_OK;
}

static int pcg_advance(nrs_ctx* c, Engine* e, double lam, int stop_level, int* it_io, bool* done) {
    while (true) {
        // Once no peek is pending, batches are sized by the previous trial's iteration count (half of
        // what it predicts is left): fewer host round trips; launches past convergence are no-ops.
        int count = 0;
        if (stop_level == 0 && e->pred_iters > *it_io) count = std::min(std::max((e->pred_iters - *it_io) / 2, c->opt.pcg_batch), 8 * c->opt.pcg_batch);
        if (stop_level == 0 && e->pred_iters >= *it_io && e->pred_iters + 1 - *it_io <= c->opt.pcg_batch) count = e->pred_iters + 1 - *it_io;   // short solves: finish in one batch
        // past what the last solve needed (its count sized the batch before, and the solve is still running): iteration counts of
        // successive trials differ by one or two, so two more at a time -- a whole default batch here was one useful launch pair and
        // seven no-ops in front of the evaluation on C2 (profiles/r10_c2_wasted_launches_parent.txt)
        if (stop_level == 0 && e->pred_iters > 0 && *it_io > e->pred_iters && e->d.plain && !e->d.sh_on && !e->d.fused) count = 2;
        if (stop_level > 0 && e->pred_peek > 0) count = std::max(2, std::min(e->pred_peek, c->opt.pcg_batch));                                // waiting for a milestone: small steps
        if (*it_io >= c->opt.pcg_max_iters) { *done = true; break; }
        NRS_TRY(pcg_enqueue_batch(c, e, lam, it_io, count, ++c->seq));      // its last launch publishes the flags
        NRS_HIP(c, hipGetLastError());
        NRS_TRY(wait_published(c, e->h_flags, c->seq, c->stream));
        if (e->h_flags[0] || *it_io >= c->opt.pcg_max_iters) { *done = true; break; }
        if (stop_level && e->h_flags[3] >= stop_level) { *done = false; break; }
    }
    return NRS_OK;
}

// size of a PCG trial's first batch (trial q of an LM iteration): up to the first peek milestone the last trial needed, or the
// whole solve the last one needed where it was short
static int first_batch(const nrs_ctx* c, const Engine* e, int q) {
    const bool expect_accept = q == 0 && e->first_trial_accepted && e->pred_iters > 0 && e->pred_iters + 1 <= 2 * c->opt.pcg_batch;
    if (!c->opt.exact_trials && !expect_accept) return e->pred_peek > 0 ? std::min(e->pred_peek, c->opt.pcg_batch) : std::max(1, c->opt.pcg_batch / 2);
    if (e->pred_iters > 0 && e->pred_iters + 1 <= 2 * c->opt.pcg_batch) return e->pred_iters + 1;
    return 0;
}

// What one engine_optimize call fixes before its first LM iteration: the switches read once per call, the shadow sets trials may use
struct LmRun {
    nrs_ctx* c; Engine* e;
    bool peek_debug, check_chi, spec_dbg;                          // NRS_PEEK_DEBUG, NRS_CHECK_CHI, NRS_SPEC_DBG (host clocks of a batch on stderr)
    bool rearm;                                                    // plain window on the two-kernel PCG: k_finalize re-arms the status words (Engine::rearm; NRS_NO_REARM: a fill per trial)
    int n_spec, n_spec_pcg;                                        // shadow sets for trials of a directly solved engine / of a PCG window (0: one trial at a time)
    int spec_first, spec_first_pcg;                                // NRS_SPEC_FIRST=<n>: followers behind the first trial of an iteration
};
static LmRun lm_run(nrs_ctx* c, Engine* e) {
    const Dev& d = e->d;
    LmRun r{c, e};
    r.peek_debug = c->dbg.is_set(SW_PEEK_DEBUG);
    r.check_chi = c->dbg.is_set(SW_CHECK_CHI);
    r.spec_dbg = c->dbg.is_set(SW_SPEC_DBG);
    // Speculative trials (directly solved single-pose engines; nrs_engine_types.hpp SpecSet): after a rejected trial the rest of the run
    // goes out as a batch -- the trial g2o would try next on the engine's own arrays, the ones after it (lam x ni, then x 2 ni, ...) on
    // the shadow sets -- and the results are read in order.  NRS_SPEC_TRIALS=0: one at a time (the same trials, the same bits).
    r.n_spec = e->nd && e->nd->on && d.K == 1 && !d.sh_on && !d.ec_on && !c->opt.profile && !c->dbg.is_set(SW_CHECK_EVAL) &&
                       e->nd->S().chain_from >= e->nd->S().plan.n_levels       // (the chained factorisation's workgroups wait for each other too: one such launch at a time)
                   ? std::min(e->n_spec, e->nd->S().n_alt) : 0;
    // ... and BA windows on the two-kernel PCG (PcgSetView): a trial of the batch is its pcg_begin, its first PCG batch and its
    // evaluation; the host then takes the trials in order through the usual peeks, further PCG batches going to the trial's own set.
    // The first batch's size depends on the milestone the trials before it reached (first_batch): a trial whose size the host does
    // not confirm when it gets to it is discarded with the rest of the batch and solved again on the engine's own arrays.
    r.n_spec_pcg = e->spec_pcg && !(e->nd && e->nd->on) && !d.sh_on && !d.fused && d.sk_n == 0 && !(e->kft && e->kft->on) &&
                           !c->opt.profile && !c->dbg.is_set(SW_CHECK_EVAL)
                       ? e->n_spec : 0;
    r.rearm = d.plain && !(e->nd && e->nd->on) && !d.sh_on && !d.fused && !d.coarse && d.sk_n == 0 && !(e->kft && e->kft->on) &&
              !c->opt.profile && !c->dbg.is_set(SW_CHECK_EVAL) && !c->dbg.is_set(SW_NO_REARM);
    r.spec_first = c->dbg.int_of(SW_SPEC_FIRST);
    r.spec_first_pcg = c->dbg.is_set(SW_SPEC_FIRST) ? r.spec_first : r.n_spec_pcg;
    return r;
}

// The LM trials in flight: the one g2o would try next (set -1: the engine's own arrays) and the ones that follow it if it is rejected
// (shadow sets 0, 1, ...), enqueued together and taken in order.
struct TrialBatch {
    struct Pending { int set; double lam; int seq; int solve_id; int first; int pit; };
    const LmRun r;
    Pending pend[1 + SPEC_MAX];
    int n_pend = 0, i_pend = 0;
    bool ok = false;                                               // (set on the regular return)
    std::chrono::steady_clock::time_point t_batch = std::chrono::steady_clock::now();
    explicit TrialBatch(const LmRun& r_) : r(r_) {}
    // an error return with trials in flight: nothing of theirs may outlive the engine the caller is about to drop
    ~TrialBatch() {
        if (!ok) for (int j = 0; j < std::max(r.n_spec, r.n_spec_pcg); ++j) if (r.c->spec_stream[j]) (void)hipStreamSynchronize(r.c->spec_stream[j].get());
    }
    bool empty() const { return i_pend == n_pend; }
    // the context's stream continues behind every shadow trial of the batch (they read the linearisation and the state)
    int join() {
        nrs_ctx* c = r.c;
        // trials of the batch nobody has asked for yet are not needed: their solves drain (the context's stream is idle here -- the
        // results before them have been read -- so the word is written at once)
        // PCG windows: one fill for the words of all sets, with the id of the last trial enqueued (Dev::abort: every trial up to it
        // is over or not needed; later ones carry larger ids)
        bool any = false;
        for (int j = i_pend; j < n_pend && !c->dbg.is_set(SW_SPEC_NO_ABORT); ++j) {
            if (pend[j].set < 0) continue;
            if (r.n_spec_pcg > 0) any = true;
            else NRS_HIP(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(r.e->spec[pend[j].set].abort), pend[j].solve_id, 1, c->stream));
        }
        if (any) NRS_HIP(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(r.e->spec[0].abort), r.e->spec_gen, r.e->n_spec, c->stream));
        for (int j = 0; j < n_pend; ++j)
            if (pend[j].set >= 0) NRS_HIP(c, hipStreamWaitEvent(c->stream, c->spec_join[pend[j].set].get(), 0));
        n_pend = i_pend = 0;
        return NRS_OK;
    }
    // the next result, which must be the trial at damping lam
    int take(double lam, const Pending** out) {
        const Pending& pp = pend[i_pend++];
        if (pp.lam != lam) return r.c->fail(NRS_ERR_STATE, "speculative trial: damping %.17g does not match the sequence (%.17g)", pp.lam, lam);
        *out = &pp;
        return NRS_OK;
    }
    // PCG window, nothing in flight: inside a run of rejections, this trial and the ones after it (may leave the batch empty: the
    // trial then goes out on its own)
    int fill_pcg(int it, int qmax, double lam, double ni) {
        nrs_ctx* c = r.c; Engine* e = r.e;
        Dev& d = e->d;                                             // (seen through each trial's PcgSetView below)
        const int trial = 1 - e->cur;
        n_pend = i_pend = 0;
        int nb = 1;
        if (qmax >= 1) nb = std::min(std::min(std::max(e->spec_run - qmax + 1, 2), 1 + r.n_spec_pcg), 10 - qmax);
        // the first trial of an iteration whose first trial was rejected last time goes out with followers (NRS_SPEC_FIRST=<n>
        // of them, default n_spec; 0: none) -- C2: the rejected run 852 -> 642 us of a step, 2.62 -> 2.48 ms per step
        if (qmax == 0 && r.spec_first_pcg > 0 && it < 32 && (e->spec_run_at >> it & 1u)) nb = std::min(1 + r.n_spec_pcg, 1 + r.spec_first_pcg);
        if (nb <= 1) return NRS_OK;
        NRS_HIP(c, hipEventRecord(c->spec_fork.get(), c->stream));
        double l = lam, n = ni;
        for (int j = 0; j < nb; ++j) {
            if (j > 0) { l *= n; n *= 2; if (!std::isfinite(l)) break; }
            Pending& p = pend[n_pend];
            // (followers of an iteration's first trial: the first batch the last run's later trials were confirmed with --
            // the milestone of a run's trials, not of the accepted trial before it that first_batch would go by)
            p.first = qmax == 0 && j > 0 && e->spec_follow_first > 0 ? e->spec_follow_first : first_batch(c, e, qmax + j);
            p.set = j - 1; p.lam = l; p.solve_id = ++e->spec_gen; p.pit = 0;
            PcgSetView v(c, e, p.set, p.solve_id);
            if (p.set >= 0) NRS_HIP(c, hipStreamWaitEvent(c->stream, c->spec_fork.get(), 0));
            NRS_TRY(pcg_begin(c, e, l, &p.pit));
            NRS_TRY(pcg_enqueue_batch(c, e, l, &p.pit, p.first));
            hipLaunchKernelGGL(k_apply, dim3(d.sh_nvb), dim3(BLK), 0, c->stream, d, l, d.pose[e->cur], d.xl[e->cur], d.pose[trial], d.xl[trial]);
            NRS_TRY(evaluate<false>(c, e, trial, false));
            p.seq = c->seq;
            if (p.set >= 0) NRS_HIP(c, hipEventRecord(c->spec_join[p.set].get(), c->stream));
            ++n_pend;
            if (r.spec_dbg) fprintf(stderr, "[spec] it %d trial %d: set %d first %d enqueued\n", it, qmax + j, p.set, p.first);
        }
        NRS_HIP(c, hipGetLastError());
        return NRS_OK;
    }
    // directly solved engine, nothing in flight: this trial and, inside a run of rejections, the ones that would follow it
    int fill_direct(int it, int qmax, double lam, double ni) {
        nrs_ctx* c = r.c;
        n_pend = i_pend = 0;
        // how many: up to the trial that is expected to be accepted -- runs repeat their length from one LM iteration, round and
        // frame to the next (c->spec_run: rejections of the last completed run) -- and two at a time beyond it; a trial of the
        // batch that turns out not to be needed holds the next linearisation up until it has drained
        int nb = 1;
        if (qmax == 0 && r.spec_first > 0) nb = std::min(1 + r.n_spec, 1 + r.spec_first);   // (experiment: NRS_SPEC_FIRST=<n> further trials behind the first of an iteration)
        if (qmax >= 1) nb = std::min(std::min(std::max(c->spec_run - qmax + 1, 2), 1 + r.n_spec), 10 - qmax);
        if (c->dbg.is_set(SW_SPEC_FIXED) && qmax >= 1) nb = std::min(std::min(std::max(1, c->dbg.int_of(SW_SPEC_FIXED)), 1 + r.n_spec), 10 - qmax);
        if (nb > 1) NRS_HIP(c, hipEventRecord(c->spec_fork.get(), c->stream));
        double l = lam, n = ni;
        const auto tq0 = std::chrono::steady_clock::now();
        for (int j = 0; j < nb; ++j) {
            if (j > 0) { l *= n; n *= 2; if (!std::isfinite(l)) break; }
            pend[n_pend].set = j - 1; pend[n_pend].lam = l;
            NRS_TRY(direct_trial_enqueue(c, r.e, j - 1, l, &pend[n_pend].seq, &pend[n_pend].solve_id, nb > 1));
            ++n_pend;
            if (r.spec_dbg) fprintf(stderr, "[spec] it %d trial %d: set %d enqueued at +%.1f us\n", it, qmax, j - 1, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tq0).count());
        }
        NRS_HIP(c, hipGetLastError());
        t_batch = tq0;
        return NRS_OK;
    }
};

// trial state, chi2 and scale of the solve so far, read back with one synchronisation (chi2, scale and the PCG flags)
static int eval_trial(nrs_ctx* c, Engine* e, double lam) {
    const Dev& d = e->d;
    const int trial = 1 - e->cur;
    Timer t(c, &c->prof.update_ms, &c->prof.update_launches);
    const bool one_pose = d.K == 1 && !d.sh_on;                    // a2's engines: trial state and reprojection chi2 in one launch
    if (one_pose)
        hipLaunchKernelGGL(k_apply_reproj, dim3(((d.sh_ng + 7) / 8) * 8), dim3(BLK), 0, c->stream, d, lam, d.pose[e->cur], d.xl[e->cur], d.pose[trial], d.xl[trial]);
    else
        hipLaunchKernelGGL(k_apply, dim3(d.sh_nvb), dim3(BLK), 0, c->stream, d, lam, d.pose[e->cur], d.xl[e->cur], d.pose[trial], d.xl[trial]);
    if (d.sh_on) NRS_TRY(c->comm->exchange(c, d.xl[trial], e->halo, c->stream));   // the regularisers read the neighbours' boundary keyframes
    NRS_TRY(evaluate<false>(c, e, trial, one_pose));
    NRS_TRY(wait_published(c, e->h_flags, c->seq, c->stream));
    if (c->dbg.is_set(SW_CHECK_EVAL)) {                                // (debug: the same evaluation again on the same state must give the same bits)
        const double chi1 = e->h_scal[SC_CHI], sc1 = e->h_scal[SC_SCALE];
        NRS_TRY(evaluate<false>(c, e, trial, false));
        NRS_TRY(wait_published(c, e->h_flags, c->seq, c->stream));
        if (e->h_scal[SC_CHI] != chi1 || e->h_scal[SC_SCALE] != sc1)
            fprintf(stderr, "[nrs] evaluation not reproducible: chi2 %.17g / %.17g, scale %.17g / %.17g\n", chi1, e->h_scal[SC_CHI], sc1, e->h_scal[SC_SCALE]);
    }
    return NRS_OK;
}

// One LM trial at damping lam -- g2o's solve + update + computeActiveErrors (optimization_algorithm_levenberg.cpp:98-119) -- from
// pcg_begin, or the hand-over from the batch, to its final figures.
struct LmTrial {
    double chi_new = 0, scale = 0;                                 // chi2 at the trial state; the gain ratio's denominator (computeScale + 1e-3)
    bool early = false;                                            // rejected at a peek: the solve was not finished
    int status = 0, inner = 0, peek_it = 0, pit = 0;               // the solve's flags[2] (0: fine), flags[1] (iterations), flags[4] (iterations to the first milestone); enqueued
    int set = -1;                                                  // the shadow set that holds the trial state (-1: the engine's own arrays)
};
static int run_trial(const LmRun& r, TrialBatch& tb, int it, int qmax, double lam, double ni, double chi, LmTrial* out) {
    nrs_ctx* c = r.c; Engine* e = r.e;
    int pit = 0, spec_seq = 0, spec_id = 0;
    int won = -1;                                                  // the shadow set that holds this trial's state (-1: the engine's own)
    bool done = false, early = false;
    bool in_flight = false;                                        // PCG window: this trial's first batch and evaluation went out with a batch
    double temp = 0, scale = 0;
    const bool direct = e->nd && e->nd->on;                        // nested-dissection Cholesky instead of PCG (nrs_engine_nd.hpp)
    const double *hs = e->h_scal; const int* hf = e->h_flags;      // the mirrors this trial's results arrive in
    if (r.n_spec_pcg > 0) {
        if (tb.empty()) NRS_TRY(tb.fill_pcg(it, qmax, lam, ni));
        if (qmax > 0) e->spec_follow_first = first_batch(c, e, qmax);
        if (!tb.empty()) {
            const TrialBatch::Pending* pp = nullptr;
            NRS_TRY(tb.take(lam, &pp));
            // (exact trials evaluate the converged solve only: where its batches end does not matter)
            if (!c->opt.exact_trials && pp->first != first_batch(c, e, qmax)) {
                if (r.spec_dbg) fprintf(stderr, "[spec] it %d trial %d: first batch %d, now %d: solved again\n", it, qmax, pp->first, first_batch(c, e, qmax));
                --tb.i_pend;
                NRS_TRY(tb.join());
            } else {
                won = pp->set; pit = pp->pit; spec_seq = pp->seq; spec_id = pp->solve_id; in_flight = true;
            }
        }
    }
    {
    PcgSetView view(c, e, r.n_spec_pcg > 0 ? won : -1, spec_id);
    if (won >= 0) { hs = e->h_scal; hf = e->h_flags; }
    // (a directly solved engine's flag words are cleared by the evaluation that published them: k_finalize, every trial and linearisation)
    if (!direct && !in_flight) NRS_TRY(pcg_begin(c, e, lam, &pit));
    const bool peeking = !c->opt.exact_trials;
    // The first batch of PCG iterations and a speculative evaluation of its result go out together: most trials are decided by it
    // (converged, or clearly rejected at a peek).  Its size is what the previous trial needed to reach the first milestone (the
    // kernels record it), so a trial that is going to be rejected costs a handful of iterations.
    int seen = 0;                                                  // peek levels already evaluated
    if (direct && r.n_spec > 0) {
        if (tb.empty()) NRS_TRY(tb.fill_direct(it, qmax, lam, ni));
        const TrialBatch::Pending* pp = nullptr;
        NRS_TRY(tb.take(lam, &pp));
        won = pp->set;
        if (won >= 0) { hs = e->spec[won].h_scal; hf = e->spec[won].h_flags; }
        NRS_TRY(wait_published(c, hf, pp->seq, won >= 0 ? c->spec_stream[won].get() : c->stream));
        if (r.spec_dbg) fprintf(stderr, "[spec] it %d trial %d: result of set %d at +%.1f us\n", it, qmax, won, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tb.t_batch).count());
        done = true;
    } else if (direct) {
        // g2o's own sequence: factorise (H + lambda I), solve, evaluate (linear_solver_eigen.h:92-136); a pivot that is not
        // positive raises flags[2] and the trial counts as failed below
        NRS_TRY(nd_solve_enqueue(c, e->nd->S(), lam));
        NRS_TRY(eval_trial(c, e, lam));
        done = true;
    } else if (in_flight) {                                        // (enqueued with the batch: its publication is the one to wait for)
        NRS_TRY(wait_published(c, hf, spec_seq, c->stream));
        done = hf[0] != 0 || pit >= c->opt.pcg_max_iters;
    } else {
        // (after an iteration whose first trial was accepted, the next first trial usually is too:
        // short solves then go out whole, without the intermediate look)
        NRS_TRY(pcg_enqueue_batch(c, e, lam, &pit, first_batch(c, e, qmax)));
        NRS_TRY(eval_trial(c, e, lam));
        done = e->h_flags[0] != 0 || pit >= c->opt.pcg_max_iters;
    }
    while (true) {
        temp = hs[SC_CHI];
        scale = hs[SC_SCALE] + 1e-3;
        if (done) break;
        const int lvl = hf[3];
        if (peeking && lvl > seen) {
            // peek: a trial that is clearly going to be rejected is not solved any further -- its step is discarded, so the iterate
            // sequence is the reference's either way
            const double rho_peek = (chi - temp) / scale;
            // ... and only when the chi2 increase is well above the noise floor of the fp32 projection (relative 1e-7 per evaluation): near
            // convergence the gain ratio of a tiny step is noise over the 1e-3 regulariser of its denominator, at any accuracy
            early = hf[2] == 0 && std::isfinite(temp) && rho_peek < PEEK_RHO_LVL[lvl] && (temp - chi) > PEEK_MIN_REL_INCREASE * chi;
            if (r.peek_debug) { fprintf(stderr, "[peek] it %d trial %d lvl %d pit %d rho %.4f relinc %.3e\n", it, qmax, lvl, pit, rho_peek, (temp - chi) / chi); early = false; }
            if (early) break;
            seen = lvl;
            // the remaining looks exist only to reject: a gain ratio this far above every threshold cannot get there any more
            // (estimates are within ~0.15), so the solve runs to convergence without further interruptions
            if (rho_peek > 0.25 && !r.peek_debug) seen = PEEK_LEVELS;
        }
        NRS_TRY(pcg_advance(c, e, lam, peeking && seen < PEEK_LEVELS ? seen + 1 : 0, &pit, &done));
        NRS_TRY(eval_trial(c, e, lam));
    }
    }                                                              // (the engine's own view again: the caller may swap the state)
    // (flags[2] == 2: a bounded wait of the direct solver ran out -- a synchronisation fault, not a matrix that is not positive
    // definite: the factor and the assembly areas hold partial data, so this is an error, never a rejected trial)
    if (hf[2] == 2) return c->fail(NRS_ERR_HIP, "direct solve: a wait for another workgroup's result timed out (LM iteration %d, trial %d, solve set %d)", it, qmax, won);
    // (the last publication was an evaluation's: it left the words of a finished solve cleared)
    if (e->rearm && !direct) e->flags_clean[1 + won] = hf[0] != 0;
    out->chi_new = temp; out->scale = scale; out->early = early;
    out->status = hf[2]; out->inner = hf[1]; out->peek_it = hf[4];
    out->set = won; out->pit = pit;
    return NRS_OK;
}

// g2o SparseOptimizer::optimize + OptimizationAlgorithmLevenberg::solve on the resident problem
// (sparse_optimizer.cpp:203-285, optimization_algorithm_levenberg.cpp:57-174).
// trace->count / iterations are accumulated (the drivers reset them once per entry point).
int engine_optimize(nrs_ctx* c, Engine* e, int iters, int round, nrs_lm_trace* trace) {
    if (iters < 0) return c->fail(NRS_ERR_INVALID, "iters < 0");
    NRS_HIP(c, hipSetDevice(c->device));
    Dev& d = e->d;
    const LmRun run = lm_run(c, e);
    e->rearm = run.rearm;
    for (bool& f : e->flags_clean) f = false;                      // (whatever touched the words since the last call: the first linearisation clears them)
    TrialBatch batch(run);
    double lam = -1, ni = 2;
    double chi_carry = 0;
    for (int it = 0; it < iters; ++it) {
        NRS_TRY(evaluate<true>(c, e, e->cur));                     // buildSystem (levenberg.cpp:83)
        // computeActiveErrors at the start of an iteration re-derives the chi2 the last accepted trial already produced (same state, same
        // summation order): after the first iteration the host does not wait for it, the linearisation and the first PCG batch go out back to back
        double chi = chi_carry;
        if (it == 0 || run.check_chi) {
            NRS_TRY(wait_published(c, e->h_flags, c->seq, c->stream));
            if (run.check_chi && it > 0 && e->h_scal[SC_CHI] != chi_carry)
                fprintf(stderr, "[nrs] chi2 carried %.17g vs recomputed %.17g\n", chi_carry, e->h_scal[SC_CHI]);
            chi = e->h_scal[SC_CHI];
        }
        if (it == 0) { lam = 1e-5 * e->h_scal[SC_MAXDIAG]; ni = 2; }   // computeLambdaInit: tau * max diagonal (levenberg.cpp:89-91, 153-165)
        if (!std::isfinite(chi) || !std::isfinite(lam)) return c->fail(NRS_ERR_NUMERIC, "non-finite chi2/lambda at LM iteration %d", it);
        double rho = 0;
        int qmax = 0;
        do {                                                       // levenberg.cpp:97-145
            const int trial = 1 - e->cur;
            LmTrial t;
            NRS_TRY(run_trial(run, batch, it, qmax, lam, ni, chi, &t));
            const bool ok = t.status == 0;
            double temp = t.chi_new;
            if (!t.early && !ok) temp = 1.7976931348623157e308;    // (ok2 false: tempChi = max, levenberg.cpp:121)
            if (!t.early) e->pred_iters = t.inner;
            if (t.peek_it > 0) e->pred_peek = t.peek_it;
            if (qmax == 0) e->first_trial_accepted = !t.early && (chi - temp) / t.scale > 0 && std::isfinite(temp);
            rho = (chi - temp) / t.scale;                          // levenberg.cpp:123-126
            if (run.peek_debug) fprintf(stderr, "[peek] it %d trial %d FINAL pit %d rho %.4f\n", it, qmax, t.pit, rho);
            const bool accepted = !t.early && rho > 0 && std::isfinite(temp);
            if (trace) {
                if (trace->trials && trace->count < trace->capacity) {
                    nrs_lm_trial& Tr = trace->trials[trace->count];
                    Tr.round = round; Tr.iter = it; Tr.trial = qmax; Tr.accepted = accepted; Tr.solver_ok = ok;
                    Tr.inner_iters = t.inner; Tr.early_rejected = t.early; Tr.reserved = 0;
                    Tr.lambda = lam; Tr.chi2 = chi; Tr.chi2_new = temp; Tr.rho = rho;
                }
                trace->count++;
            }
            if (accepted) {                                        // levenberg.cpp:128-137
                double alpha = 1.0 - std::pow(2 * rho - 1, 3);
                alpha = std::min(alpha, 2.0 / 3.0);
                lam *= std::max(1.0 / 3.0, alpha);
                ni = 2;
                chi = temp;
                if (t.set >= 0) {                                  // (the state sits in the shadow set's arrays: they become the engine's, the engine's the set's)
                    std::swap(d.pose[trial], e->spec[t.set].pose);
                    std::swap(d.xl[trial], e->spec[t.set].xl);
                }
                NRS_TRY(batch.join());                             // (trials of the batch still in flight are discarded; the next linearisation waits for them)
                if (run.n_spec > 0 && qmax > 0) c->spec_run = qmax;   // (a run of qmax rejections ended here)
                if (run.n_spec_pcg > 0) {
                    if (qmax > 0) e->spec_run = qmax;
                    if (it < 32) e->spec_run_at = qmax > 0 ? e->spec_run_at | 1u << it : e->spec_run_at & ~(1u << it);
                }
                e->cur = trial;                                    // discardTop: the trial state becomes current
            } else {                                               // levenberg.cpp:138-143
                lam *= ni;
                ni *= 2;                                           // pop: current state untouched
                if (!std::isfinite(lam)) break;
            }
            ++qmax;
        } while (rho < 0 && qmax < 10);                            // levenberg.cpp:144 (_maxTrialsAfterFailure = 10)
        NRS_TRY(batch.join());
        chi_carry = chi;
        if (trace) trace->iterations++;
        if (qmax == 10 || rho == 0 || !std::isfinite(lam)) break;   // levenberg.cpp:147-150: no valid step: terminate
    }
    batch.ok = true;
    return NRS_OK;
}

// sharded: the current estimates of all rows on every rank (each rank contributes its own rows, zeros
// elsewhere, summed over the ranks); uses the PCG vectors w and s as scratch
static int gather_state(nrs_ctx* c, Engine* e, const double** xl_full, size_t extra_bytes = 0) {   // extra_bytes: room behind the two vectors (row-limited ranks: the taps' full-length flags / observations)
    Dev& d = e->d;
    *xl_full = d.xl[e->cur];
    if (!d.sh_on) return NRS_OK;
    const size_t n = 3 * (size_t)d.n_rows;
    double *in = d.wv, *out = d.sv;
    if (d.row_hi - d.row_lo < d.n_rows) {                         // the rank holds its own rows of the vectors only: full-length scratch for the duration of the call
        NRS_TRY(c->ensure(c->gather_ws, 2 * sizeof(double) * n + extra_bytes));
        in = c->gather_ws.as<double>(); out = in + n;
    }
    hipLaunchKernelGGL(k_mask_rows, dim3((unsigned)((n + BLK - 1) / BLK)), dim3(BLK), 0, c->stream, d, d.xl[e->cur], in);
    NRS_HIP(c, hipGetLastError());
    NRS_TRY(c->comm->allreduce(c, in, out, n));
    *xl_full = out;
    return NRS_OK;
}

int engine_download(nrs_ctx* c, Engine* e, Pose* poses, double* x) {
    Dev& d = e->d;
    std::vector<double> xl((size_t)d.n_rows * 3);
    const double* src = nullptr;
    NRS_TRY(gather_state(c, e, &src));
    if (poses) NRS_HIP(c, hipMemcpyAsync(poses, d.pose[e->cur], sizeof(Pose) * d.K, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(xl.data(), src, sizeof(double) * xl.size(), hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    c->gather_ws.reset();
    if (x)
        for (int v = 0; v < d.M; ++v)
            for (int k = 0; k < 3; ++k) x[3 * (size_t)v + k] = xl[3 * (size_t)e->vrow[v] + k];
    return NRS_OK;
}

int engine_residuals(nrs_ctx* c, Engine* e, double* r_reproj, double* r_spring, double* r_damper) {
    Dev& d = e->d;
    // the taps read the edges by vertex (not the packed incidence records): their device copies and the output block live in a
    // context buffer that is filled when an engine is first asked for residuals (BA windows that never are hold none of it)
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_vrow = 0, o_sp = o_vrow + al(sizeof(int) * (size_t)d.M), o_dm = o_sp + al(sizeof(int) * 2 * (size_t)d.n_sp),
                 o_d0 = o_dm + al(sizeof(int) * 4 * (size_t)d.n_dm), o_w = o_d0 + al(sizeof(float) * (size_t)d.n_sp),
                 o_out = o_w + al(sizeof(float) * (size_t)d.n_dm),
                 total = o_out + sizeof(double) * (2 * (size_t)d.M + (size_t)d.n_sp + 3 * (size_t)d.n_dm);
    if (total > c->tap.cap || !c->tap.p) { c->tap_serial = 0; NRS_TRY(c->ensure(c->tap, total)); }
    char* tb = c->tap.as<char>();
    int *t_vrow = reinterpret_cast<int*>(tb + o_vrow), *t_sp = reinterpret_cast<int*>(tb + o_sp), *t_dm = reinterpret_cast<int*>(tb + o_dm);
    float *t_d0 = reinterpret_cast<float*>(tb + o_d0), *t_w = reinterpret_cast<float*>(tb + o_w);
    if (c->tap_serial != e->serial) {
        NRS_HIP(c, hipMemcpyAsync(t_vrow, e->vrow.data(), sizeof(int) * (size_t)d.M, hipMemcpyHostToDevice, c->stream));
        const hipMemcpyKind kd = e->dev_edges ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        const int* src_sp = e->dev_edges ? e->raw_sp : e->sp_ij.data();
        const float* src_d0 = e->dev_edges ? e->raw_d0 : e->sp_d0.data();
        const int* src_dm = e->dev_edges ? e->raw_dm : e->dm_idx.data();
        const float* src_w = e->dev_edges ? e->raw_w : e->dm_w.data();
        if (d.n_sp) NRS_HIP(c, hipMemcpyAsync(t_sp, src_sp, sizeof(int) * 2 * (size_t)d.n_sp, kd, c->stream));
        if (d.n_sp) NRS_HIP(c, hipMemcpyAsync(t_d0, src_d0, sizeof(float) * (size_t)d.n_sp, kd, c->stream));
        if (d.n_dm) NRS_HIP(c, hipMemcpyAsync(t_dm, src_dm, sizeof(int) * 4 * (size_t)d.n_dm, kd, c->stream));
        if (d.n_dm) NRS_HIP(c, hipMemcpyAsync(t_w, src_w, sizeof(float) * (size_t)d.n_dm, kd, c->stream));
        c->tap_serial = e->serial;
    }
    double* rr = reinterpret_cast<double*>(tb + o_out);
    double* rs = rr + 2 * (size_t)d.M;
    double* rd = rs + (size_t)d.n_sp;
    const int n = std::max(d.M, std::max(d.n_sp, d.n_dm));
    const double* xl_full = nullptr;
    const bool limited = d.row_hi - d.row_lo < d.n_rows;           // a rank of a sharded window holds its own rows only: the tap reads every row's flag and observation
    if (limited && d.X0) return c->fail(NRS_ERR_STATE, "residual taps: a sharded window with offsets is not supported");
    NRS_TRY(gather_state(c, e, &xl_full, limited ? 9 * (size_t)d.n_rows + 256 : 0));
    const uint8_t* t_rflag = d.rflag;
    const float* t_uv = d.uv;
    if (limited) {
        char* xb = c->gather_ws.as<char>() + 2 * sizeof(double) * 3 * (size_t)d.n_rows;
        float* fu = reinterpret_cast<float*>(xb);
        uint8_t* fr = reinterpret_cast<uint8_t*>(xb + 8 * (size_t)d.n_rows);
        NRS_HIP(c, hipMemcpyAsync(fu, e->h_uv.data(), sizeof(float) * 2 * (size_t)d.n_rows, hipMemcpyHostToDevice, c->stream));
        NRS_HIP(c, hipMemcpyAsync(fr, e->h_rflag.data(), (size_t)d.n_rows, hipMemcpyHostToDevice, c->stream));
        t_rflag = fr; t_uv = fu;
    }
    hipLaunchKernelGGL(k_tap_residuals, dim3((n + 255) / 256), dim3(256), 0, c->stream, d, d.pose[e->cur], xl_full, t_rflag, t_uv,
                       t_vrow, t_sp, t_d0, t_dm, t_w, rr, rs, rd);
    NRS_HIP(c, hipGetLastError());
    if (r_reproj) NRS_HIP(c, hipMemcpyAsync(r_reproj, rr, sizeof(double) * 2 * (size_t)d.M, hipMemcpyDeviceToHost, c->stream));
    if (r_spring && d.n_sp) NRS_HIP(c, hipMemcpyAsync(r_spring, rs, sizeof(double) * (size_t)d.n_sp, hipMemcpyDeviceToHost, c->stream));
    if (r_damper && d.n_dm) NRS_HIP(c, hipMemcpyAsync(r_damper, rd, sizeof(double) * 3 * (size_t)d.n_dm, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    c->gather_ws.reset();
    return NRS_OK;
}

int engine_edge_chi2(nrs_ctx* c, Engine* e, double* reproj, double* spring, double* damper) {
    Dev& d = e->d;
    std::vector<double> rr(2 * (size_t)d.M), rs((size_t)d.n_sp), rd(3 * (size_t)d.n_dm);
    NRS_TRY(engine_residuals(c, e, rr.data(), rs.data(), rd.data()));
    if (reproj)
        for (int i = 0; i < d.M; ++i) reproj[i] = d.info_reproj * (rr[2 * i] * rr[2 * i] + rr[2 * i + 1] * rr[2 * i + 1]);
    if (spring)
        for (int i = 0; i < d.n_sp; ++i) spring[i] = d.info_pos * rs[i] * rs[i];
    if (damper)
        for (int i = 0; i < d.n_dm; ++i)
            damper[i] = d.info_spatial * (rd[3 * i] * rd[3 * i] + rd[3 * i + 1] * rd[3 * i + 1] + rd[3 * i + 2] * rd[3 * i + 2]);
    return NRS_OK;
}

// parity tap of the problem construction: FNV-1a checksums of every packed array of the resident problem (host or device
// built: the two must agree bit for bit), out[0..24)
int engine_pack_hash(nrs_ctx* c, Engine* e, uint64_t* out) {
    const Dev& d = e->d;
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    auto fnv = [](const void* p, size_t n) {
        uint64_t h = 1469598103934665603ULL;
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ULL; }
        return h;
    };
    std::vector<char> buf;
    auto dev = [&](const void* p, size_t bytes, uint64_t* o) {
        buf.resize(std::max<size_t>(bytes, 1));
        if (bytes && hipMemcpy(buf.data(), p, bytes, hipMemcpyDeviceToHost) != hipSuccess) return false;
        *o = fnv(buf.data(), bytes);
        return true;
    };
    for (int i = 0; i < 24; ++i) out[i] = 0;
    const size_t ns = (size_t)d.n_rows / (64 / d.T), nt = (size_t)d.n_regblk;
    std::vector<int> hp(nt + 1);
    NRS_HIP(c, hipMemcpy(hp.data(), d.halo_ptr, sizeof(int) * (nt + 1), hipMemcpyDeviceToHost));
    const size_t n_halo = (size_t)hp[nt];
    bool ok = true;
    out[0] = fnv(e->vrow.data(), sizeof(int) * e->vrow.size());
    ok = ok && dev(d.ss_ptr, sizeof(int) * (ns + 1), &out[1]) && dev(d.sd_ptr, sizeof(int) * (ns + 1), &out[2]);
    ok = ok && dev(d.s_om, sizeof(uint32_t) * (size_t)d.ss_nnz, &out[3]) && dev(d.s_d0, sizeof(float) * (size_t)d.ss_nnz, &out[4]);
    ok = ok && dev(d.d_hdr, sizeof(uint2) * (size_t)d.sd_nnz, &out[5]) && dev(d.d_w, sizeof(float) * (size_t)d.sd_nnz, &out[6]);
    out[7] = fnv(hp.data(), sizeof(int) * hp.size());
    ok = ok && dev(d.halo_rows, sizeof(int) * n_halo, &out[8]) && dev(d.halo_ns, sizeof(int) * nt, &out[9]) && dev(d.tile_list, sizeof(int) * nt, &out[10]);
    if (d.ec_on) {
        std::vector<EcSpring> es((size_t)d.ec_nsp);
        std::vector<EcDamper> ed((size_t)d.ec_ndm);
        if (d.ec_nsp) NRS_HIP(c, hipMemcpy(es.data(), d.ec_sp, sizeof(EcSpring) * es.size(), hipMemcpyDeviceToHost));
        if (d.ec_ndm) NRS_HIP(c, hipMemcpy(ed.data(), d.ec_dm, sizeof(EcDamper) * ed.size(), hipMemcpyDeviceToHost));
        for (auto& x : es) x.pad = 0;
        out[11] = fnv(es.data(), sizeof(EcSpring) * es.size());
        out[12] = fnv(ed.data(), sizeof(EcDamper) * ed.size());
        ok = ok && dev(d.ec_w, sizeof(float) * (size_t)d.ec_ndm, &out[13]);
    }
    // per-row arrays: the rows this engine holds (all of them, except on a row-limited rank of a sharded window: ArenaPlan::get_rows)
    const size_t r0 = (size_t)d.row_lo, rn = (size_t)(d.row_hi - d.row_lo);
    ok = ok && dev(d.rflag + r0, rn, &out[14]) && dev(d.uv + 2 * r0, sizeof(float) * 2 * rn, &out[15]);
    ok = ok && dev(d.xl_init + 3 * r0, sizeof(double) * 3 * rn, &out[16]) && dev(d.pose_init, sizeof(Pose) * (size_t)d.K, &out[17]);
    ok = ok && dev(d.grp_pose, sizeof(int) * (size_t)d.n_groups, &out[18]) && dev(d.pose_grp_ptr, sizeof(int) * ((size_t)d.K + 1), &out[19]);
    const int sc[16] = {d.n_rows, d.T, d.ss_nnz, d.sd_nnz, d.max_halo, d.max_halo_s, d.n_tiles_cls[0], d.n_tiles_cls[1], d.cap_h[0], d.cap_h[1], d.cap_s[0], d.cap_s[1],
                        d.ec_nblk, d.lin_rb, d.hier + 2 * d.fused + 4 * d.ecd + 8 * d.use_lds, d.plain + 2 * d.tp_ok + 4 * d.h4};
    if (d.plain) { uint64_t h = 0; ok = ok && dev(d.row_tp + r0, sizeof(uint32_t) * rn, &h); out[20] ^= h * 31; }
    if (d.plain) { uint64_t h = 0; ok = ok && dev(d.row_cnt + r0, sizeof(uint32_t) * rn, &h); out[20] ^= h * 131; }
    out[20] ^= fnv(sc, sizeof(sc));
    out[21] = e->dev_edges ? 1 : 0;                                  // (which path built it: not part of the comparison)
    if (d.fused) ok = ok && dev(d.tile_desc, sizeof(int) * 8 * nt, &out[22]) && dev(d.halo_fix, sizeof(int) * BLK * nt, &out[23]);
    else if (d.plain && d.use_lds) ok = ok && dev(d.halo_fix, sizeof(int) * HALO_FIX * nt, &out[23]);
    if (!ok) return c->fail(NRS_ERR_HIP, "pack hash: a device copy failed");
    return NRS_OK;
}

int engine_gradient(nrs_ctx* c, Engine* e, double* b, double* diag) {
    Dev& d = e->d;
    if (d.sh_on) return c->fail(NRS_ERR_STATE, "the gradient tap is not available on a sharded problem");
    NRS_TRY(evaluate<true>(c, e, e->cur));
    std::vector<double> bp(6 * (size_t)d.K), Hpp(21 * (size_t)d.K), bl(3 * (size_t)d.n_rows), D(6 * (size_t)d.n_rows);
    NRS_HIP(c, hipMemcpyAsync(bp.data(), d.bp, sizeof(double) * bp.size(), hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(Hpp.data(), d.Hpp, sizeof(double) * Hpp.size(), hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(bl.data(), d.bl, sizeof(double) * bl.size(), hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(D.data(), d.D, sizeof(double) * D.size(), hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    static const int dg[6] = {0, 6, 11, 15, 18, 20};
    for (int k = 0; k < d.K; ++k)
        for (int a = 0; a < 6; ++a) { b[6 * k + a] = bp[6 * k + a]; diag[6 * k + a] = Hpp[21 * k + dg[a]]; }
    static const int d3[3] = {0, 3, 5};
    for (int v = 0; v < d.M; ++v) {
        const size_t row = (size_t)e->vrow[v];
        for (int a = 0; a < 3; ++a) {
            b[6 * (size_t)d.K + 3 * (size_t)v + a] = bl[3 * row + a];
            diag[6 * (size_t)d.K + 3 * (size_t)v + a] = D[6 * row + d3[a]];
        }
    }
    return NRS_OK;
}

// Parity tap for the linear solve (a18): the reference's known-answer test hands its solver an explicit
// block-sparse SPD matrix (third_party/g2o/unit_test/solver/linear_solver_test.cpp:72-85).  A matrix with one
// 6x6 block coupled to 3x3 diagonal blocks is exactly what the stored-block operator path represents (H_pp,
// H_pl, D), so the blocks are written where the lineariser would have put them and the product's own kernels
// (k_trial_setup: inv3_sym / inv6_spd preconditioner, k_spmv, k_reduce_partials, k_pcg_update) solve it.
int engine_debug_solve(nrs_ctx* c, Engine* e, const double* Hpp21, const double* bp, const double* D6, const double* Hpl18,
                       const double* bl, double lam, double* xp, double* xl, int* iters, int* ok) {
    Dev& d = e->d;
    if (d.K != 1 || d.use_lds || d.fused || d.sh_on) return c->fail(NRS_ERR_STATE, "debug solve: needs a single-pose, stored-block engine");
    NRS_HIP(c, hipSetDevice(c->device));
    const size_t nr = (size_t)d.n_rows;
    std::vector<double> hD(6 * nr, 0.0), hH(18 * nr, 0.0), hb(3 * nr, 0.0);
    for (size_t r = 0; r < nr; ++r) { hD[6 * r] = hD[6 * r + 3] = hD[6 * r + 5] = 1.0; }        // padding rows: identity (lam may be 0 here)
    for (int v = 0; v < d.M; ++v) {
        const size_t row = (size_t)e->vrow[v];
        for (int k = 0; k < 6; ++k) hD[6 * row + k] = D6[6 * (size_t)v + k];
        for (int k = 0; k < 18; ++k) hH[(size_t)k * nr + row] = Hpl18[18 * (size_t)v + k];      // component-major on the device
        for (int k = 0; k < 3; ++k) hb[3 * row + k] = bl[3 * (size_t)v + k];
    }
    // rows of the caller are free variables; padding rows stay identity rows (zero blocks, zero right-hand side)
    std::vector<uint8_t> rf(nr, RF_FIXED);
    for (int v = 0; v < d.M; ++v) rf[e->vrow[v]] = 0;
    NRS_HIP(c, hipMemcpyAsync(d.rflag, rf.data(), nr, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(d.D, hD.data(), sizeof(double) * hD.size(), hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(d.Hpl, hH.data(), sizeof(double) * hH.size(), hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(d.bl, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(d.Hpp, Hpp21, sizeof(double) * 21, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(d.bp, bp, sizeof(double) * 6, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    int pit = 0;
    bool done = false;
    e->pred_iters = 0; e->pred_peek = 0;
    e->rearm = false;
    NRS_TRY(pcg_begin(c, e, lam, &pit));
    NRS_TRY(pcg_advance(c, e, lam, 0, &pit, &done));
    if (iters) *iters = e->h_flags[1];
    if (ok) *ok = e->h_flags[2] == 0 && e->h_flags[0] != 0;
    std::vector<double> hx(3 * nr);
    NRS_HIP(c, hipMemcpyAsync(xp, d.xp, sizeof(double) * 6, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(hx.data(), d.xv, sizeof(double) * hx.size(), hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    for (int v = 0; v < d.M; ++v)
        for (int k = 0; k < 3; ++k) xl[3 * (size_t)v + k] = hx[3 * (size_t)e->vrow[v] + k];
    return NRS_OK;
}

}  // namespace nrs

#include "nrs_engine_kft_debug.hpp"
