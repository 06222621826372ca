// C ABI of the AMP decoder on a design plan (amp_plan.hpp): engine choice, batched decode, the design
// operators Ab / Az, the encoder, soft output, the integrated AMP <-> BP loop, error counting.
#include <optional>
#include <type_traits>

#include "amp_plan.hpp"
#include "integ_loop.hpp"

namespace sg {

// The split engine (amp_cw2.hip) runs the per-codeword engine's iterations
// when its tables were built; SG_AMP_CW2=0 keeps the one-workgroup form
// (A/B tests).
static bool use_cw2(const sg_amp_plan *p) {
    if (!p->cw2OT) return false;
    const char *e = std::getenv("SG_AMP_CW2");
    return !(e && std::strcmp(e, "0") == 0);
}

// Engine choice for a decode of B codewords: the per-codeword engine keeps
// one workgroup per codeword, so it wants a batch that fills the CUs.
// SG_AMP_ENGINE=cw / staged forces either at decode time (tests, A/B).
static bool use_cw(const sg_amp_plan *p, int B) {
    if (!p->cw) return false;
    const char *e = std::getenv("SG_AMP_ENGINE");
    if (e && std::strcmp(e, "cw") == 0) return true;
    if (e && std::strcmp(e, "staged") == 0) return false;
    // one workgroup per codeword and CU: worth it when the batch fills whole
    // waves of the CUs (at B = CUs it is ~11 % ahead of the staged engine,
    // which keeps every CU busy at any B)
    const int cu = std::max(p->cus_assumed > 0 ? p->cus_assumed : device_cu_count(), 1);
    const int waves = (B + cu - 1) / cu;
    return B >= cu && (double)B / ((double)waves * cu) >= 0.9;
}

// The plan a decode of B codewords runs on: the companion P = 16384 plan when
// the automatic choice is the staged engine from the first iteration (the
// SG_AMP_ENGINE overrides keep the plan itself, for same-table A/B tests).
static sg_amp_plan *decode_plan(sg_amp_plan *p, int B) {
    if (!p->alt) return p;
    const char *e = std::getenv("SG_AMP_ENGINE");
    if (e && (std::strcmp(e, "cw") == 0 || std::strcmp(e, "staged") == 0)) return p;
    return use_cw(p, B) ? p : p->alt;
}

// Active-flag poll, one iteration behind the launches: the copy of the flags
// after iteration t is requested behind t's launches, iteration t + 1 is
// launched, and only then does the host wait for the copy -- the GPU works on
// t + 1 meanwhile, so the poll leaves no idle gap on the stream (a synchronous
// poll cost ~40 us of idle GPU each time, profiles/README.md).  Decisions
// taken from the flags after t apply from iteration t + 2 on, at every run and
// rank count alike (the decode stays deterministic).
struct ActivePoll {
    sg_amp_plan *p;
    int B;
    hipStream_t s;
    bool pending = false;
    const int32_t *flags = nullptr;  // the flags polled: the plan's ws_active, or a loop's own
    // pipelined decode (Cw2Pipe): each half's flags are copied on the half's own stream, behind its iteration t
    // and before its iteration t + 1 as on one stream; the second stream, which runs behind, then waits for
    // the first half's copy (ev2) and records the one event the host waits for
    hipStream_t s2 = nullptr;
    hipEvent_t ev2 = nullptr;
    int nA = 0;  // codewords of the first half
    int request() {  // behind the launches already on the stream (both streams of a pipelined decode)
        if (!p->poll_ev) SG_HIP(hipEventCreateWithFlags(&p->poll_ev, hipEventDisableTiming));
        if (p->h_active_cap < B) {
            if (p->h_active) {
                SG_HIP(hipEventSynchronize(p->poll_ev));
                SG_HIP(hipHostFree(p->h_active));
                p->h_active = nullptr;
            }
            SG_HIP(hipHostMalloc((void **)&p->h_active, sizeof(int32_t) * B, hipHostMallocDefault));
            p->h_active_cap = B;
        }
        const int32_t *src = flags ? flags : p->ws_active;
        const int n1 = s2 ? nA : B;
        SG_HIP(hipMemcpyAsync(p->h_active, src, sizeof(int32_t) * n1, hipMemcpyDeviceToHost, s));
        if (s2) {
            SG_HIP(hipEventRecord(ev2, s));
            SG_HIP(hipMemcpyAsync(p->h_active + n1, src + n1, sizeof(int32_t) * (B - n1), hipMemcpyDeviceToHost, s2));
            SG_HIP(hipStreamWaitEvent(s2, ev2, 0));
        }
        SG_HIP(hipEventRecord(p->poll_ev, s2 ? s2 : s));
        pending = true;
        return SG_OK;
    }
    // the number of active codewords at the last request (-1: none pending)
    int collect(int *n_active) {
        *n_active = -1;
        if (!pending) return SG_OK;
        SG_HIP(hipEventSynchronize(p->poll_ev));
        pending = false;
        int na = 0;
        for (int b = 0; b < B; ++b) na += p->h_active[b] != 0;
        *n_active = na;
        return SG_OK;
    }
    // One iteration of a loop that only stops on the poll: collects the flags requested an iteration ago
    // (*stopped: every codeword had stopped) and, if `due`, requests the flags behind this iteration's launches
    int step(bool due, bool *stopped) {
        int na = -1;
        SG_TRY(collect(&na));
        *stopped = na == 0;
        if (due && !*stopped) SG_TRY(request());
        return SG_OK;
    }
    // no copy into the plan's h_active outlives the loop, whichever way it is left
    ~ActivePoll() {
        if (pending) (void)hipEventSynchronize(p->poll_ev);
    }
};

// Pipelined split engine: the f32 split engine's iterations as two half-batches in flight on two streams, so
// that one half's control kernels, launch prologues and drain tails run under the other half's transforms
// (DESIGN.md "Split per-codeword engine").  Half A (the first ceil(B / 2) codewords) runs on the caller's
// stream, half B on the plan's second stream; both through the unchanged kernels on views of the per-codeword
// workspaces offset by the half's first codeword.  Every batch-level decision (poll, np 2 -> 4, hand-over, early
// end) is taken once for the whole batch at the same iteration index as on one stream, and no codeword reads
// another's state, so the results do not depend on the split.  Half B starts one launch behind: its first
// control kernel waits for half A's (a whole iteration 0 behind, so that A's cw2_ab meets B's cw2_az, measured
// 0.8 % slower: profiles/pipe_bench_ab_d194c7cc_28d51ff2.txt).  SG_AMP_PIPE=0 keeps one stream (A/B tests).
static bool use_pipe(const sg_amp_plan *p, int B) {
    const char *e = std::getenv("SG_AMP_PIPE");
    if (e && std::strcmp(e, "0") == 0) return false;
    // each half's launch (two workgroups per codeword) still puts a workgroup on every CU
    const int cu = std::max(p->cus_assumed > 0 ? p->cus_assumed : device_cu_count(), 1);
    return B >= 2 && 2 * (B / 2) >= cu;
}

struct Cw2Pipe {
    sg_amp_plan *p;
    int B, nA;
    hipStream_t sa, sb;
    bool on = false;
    enum { EV_FORK, EV_JOIN, EV_LAG, EV_POLL };
    int start() {  // after the decode's initialisation on sa
        if (!p->pipe_stream) SG_HIP(hipStreamCreateWithFlags(&p->pipe_stream, hipStreamNonBlocking));
        for (hipEvent_t &e : p->pipe_ev)
            if (!e) SG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        sb = p->pipe_stream;
        nA = (B + 1) / 2;
        prof_pipe_begin(sa);
        SG_HIP(hipEventRecord(p->pipe_ev[EV_FORK], sa));
        SG_HIP(hipStreamWaitEvent(sb, p->pipe_ev[EV_FORK], 0));
        on = true;
        p->last_piped = 1;
        return SG_OK;
    }
    // the views of codewords [c0, c0 + nb): every per-codeword array moved to its first codeword.  The partial
    // outputs and statistics keep CW2_NP parts per codeword between the halves whatever np the launch uses, so a
    // half one iteration ahead with np = 4 never writes where the other still reads with np = 2.
    void views(int c0, int nb, int t_max, Cw2Tables *tb, RegBufs<float> *bf, AmpScalars *sc) const {
        const size_t c = (size_t)c0, T = CW2_THREADS, OT = tb->OT;
        bf->B = nb;
        bf->s += c * tb->LM; bf->stM += c * tb->L; bf->stI += c * tb->L; bf->y += c * tb->n; bf->z += c * tb->n;
        bf->phi += c; bf->tau += c; bf->tau_prev += c; bf->active += c; bf->map += c * tb->L;
        if (bf->true_idx) bf->true_idx += c * tb->L;
        sc->psi += c; sc->psi_prev += c; sc->phi_prev += c; sc->gamma += c; sc->bcoef += c;
        sc->nmse += c * t_max; sc->t_final += c;
        tb->xr += c * CW2_NP * OT * T; tb->part += c * CW2_NP * tb->Lblk;
        tb->vz += c * (cw2_vz_tm((int)OT) ? cw2_otp((int)OT) : 2 * OT) * T;
        tb->ys += c * OT * T; tb->zs += c * OT * T;
        if (tb->tprof) tb->tprof += c * tb->np * 64;
    }
    int launch_iter(const RegBufs<float> &bf0, const AmpScalars &sc0, const AmpParams &pr, int t) {
        for (int h = 0; h < 2; ++h) {
            Cw2Tables tb = c2tables(p, B);
            RegBufs<float> bf = bf0;
            AmpScalars sc = sc0;
            views(h ? nA : 0, h ? B - nA : nA, pr.t_max, &tb, &bf, &sc);
            if (t == 0 && h == 1) SG_HIP(hipStreamWaitEvent(sb, p->pipe_ev[EV_LAG], 0));
            prof_pipe_half(h);
            const int rc = cw2_launch_iter(tb, bf, sc, pr, t, h ? sb : sa,
                                           t == 0 && h == 0 ? p->pipe_ev[EV_LAG] : nullptr);
            prof_pipe_half(-1);
            SG_TRY(rc);
        }
        return SG_OK;
    }
    int join() {  // half B's launches into the caller's stream; one stream from here on
        if (!on) return SG_OK;
        SG_HIP(hipEventRecord(p->pipe_ev[EV_JOIN], sb));
        SG_HIP(hipStreamWaitEvent(sa, p->pipe_ev[EV_JOIN], 0));
        on = false;
        return SG_OK;
    }
};

// What a decode is asked for, in the order of sg_amp_decode_device's arguments (results: null if not wanted)
struct DecodeArgs {
    const void *d_y; int B; const int32_t *d_true; double awgn_var; int t_max; double rtol; int phi_method;
    int32_t *d_map, *d_tfinal; double *d_nmse, *d_psi;
};

static AmpScalars scalars(const sg_amp_plan *p) {
    AmpScalars sc;
    sc.psi = p->ws_psi; sc.psi_prev = p->ws_psi_prev; sc.phi_prev = p->ws_phi_prev; sc.gamma = p->ws_gamma;
    sc.bcoef = p->ws_bco; sc.nmse = p->ws_nmse; sc.t_final = p->ws_tfinal;
    return sc;
}

static AmpParams params(const sg_amp_plan *p, const DecodeArgs &a) {
    AmpParams pr;
    pr.W = p->dW; pr.awgn_var = a.awgn_var; pr.rtol = a.rtol;
    pr.atol = 2e-15;  // 2*np.finfo(float).resolution, sparc.py:916
    pr.phi_method = a.phi_method; pr.t_max = a.t_max;
    return pr;
}

// The end of a decode: the results from the workspace to the caller's buffers
static int copy_results(const sg_amp_plan *p, const DecodeArgs &a, hipStream_t s) {
    const int B = a.B;
    if (a.d_map) SG_HIP(hipMemcpyAsync(a.d_map, p->ws_argmax, sizeof(int32_t) * B * p->L, hipMemcpyDeviceToDevice, s));
    if (a.d_tfinal) SG_HIP(hipMemcpyAsync(a.d_tfinal, p->ws_tfinal, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, s));
    if (a.d_nmse)
        SG_HIP(hipMemcpyAsync(a.d_nmse, p->ws_nmse, sizeof(double) * B * a.t_max * p->Lc, hipMemcpyDeviceToDevice, s));
    if (a.d_psi) SG_HIP(hipMemcpyAsync(a.d_psi, p->ws_psi, sizeof(double) * B * p->Lc, hipMemcpyDeviceToDevice, s));
    SG_HIP(hipGetLastError());
    return SG_OK;
}

template <typename T>
static int decode_regular(sg_amp_plan *p, const DecodeArgs &a, hipStream_t s) {
    const int B = a.B, t_max = a.t_max;
    RegTables<T> tb = rtables<T>(p);
    RegBufs<T> bf = rbufs<T>(p, B, a.d_y);
    bf.true_idx = a.d_true;
    const AmpScalars sc = scalars(p);
    const AmpParams pr = params(p, a);
    SG_TRY(reg_launch_init(B, p->Lc, t_max, p->ws_nmse, p->ws_active, p->ws_tfinal, s));
    ActivePoll poll{p, B, s};
    // f32 split engine: two workgroups per codeword (each half of the classes) while every codeword is active;
    // once the active-flag poll shows stopped codewords, four, so the dispatcher refills the CU slots of the
    // stopped ones (same box: R = 1.3 +4 %, profiles/r06_c2_parts_ab.txt; four from the start cost the
    // all-active R = 1.5 line 0.2-0.8 %: the control kernel sums twice the parts)
    p->c2_np = 2;
    // (double precision has the split engine only: SG_AMP_CW2=0 leaves it the staged engine)
    bool cw = use_cw(p, B) && (std::is_same<T, float>::value || use_cw2(p));
    p->last_engine = cw ? 2 : 1;
    p->last_handover = -1;
    p->last_piped = 0;
    Cw2Pipe pipe{p, B, 0, s, nullptr};
    if constexpr (std::is_same<T, float>::value)
        if (cw && use_cw2(p) && use_pipe(p, B) && t_max > 2) {
            SG_TRY(pipe.start());
            poll.s2 = pipe.sb;
            poll.nA = pipe.nA;
            poll.ev2 = p->pipe_ev[Cw2Pipe::EV_POLL];
        }
    const char *eng = std::getenv("SG_AMP_ENGINE");
    const bool cw_forced = eng && std::strcmp(eng, "cw") == 0;
    double handover = 0.5;  // active fraction below which the staged engine takes over
    if (const char *h = std::getenv("SG_AMP_HANDOVER"))  // tuning knob, clamped to [0, 1]
        handover = std::min(1.0, std::max(0.0, atof(h)));
    for (int t = 0; t < t_max - 1; ++t) {
        if constexpr (std::is_same<T, float>::value) {
            if (cw) {
                if (pipe.on) SG_TRY(pipe.launch_iter(bf, sc, pr, t));
                else if (use_cw2(p)) SG_TRY(cw2_launch_iter(c2tables(p, B), bf, sc, pr, t, s));
                else SG_TRY(cw_launch_iter(ctables(p, B), bf, sc, pr, t, s));
            }
        } else {
            if (cw) SG_TRY(cw2d_launch_iter(c2dtables(p), bf, sc, pr, t, s));
        }
        if (!cw) {
            if (t > 0) SG_TRY(reg_launch_ab<T>(tb, bf, s));
            SG_TRY(reg_launch_ctrl0<T>(tb, bf, sc, pr, t, s));
            SG_TRY(reg_launch_az<T>(tb, bf, t, s));
            SG_TRY(reg_launch_merge<T>(tb, bf, sc, pr, t, s));
        }
        // Poll the active flags (after iterations 3, 7, 11, ..., read one
        // iteration later, ActivePoll): stop once every codeword has stopped,
        // and hand the remaining iterations to the staged engine once half of
        // the batch has stopped -- the per-codeword engine keeps one CU per
        // codeword, so stopped codewords leave CUs idle, while the staged
        // engine spreads the active ones over every CU.  Both keep the same
        // state (s in class order, section statistics, scalars), so the
        // switch is seamless.
        int na = -1;
        SG_TRY(poll.collect(&na));  // the flags after iteration t - 1
        if (na == 0) break;
        if (na > 0 && na < B) p->c2_np = 4;
        if (na > 0 && cw && !cw_forced && na < handover * B) {
            cw = false;
            p->last_handover = t + 1;  // first iteration on the staged engine
            SG_TRY(pipe.join());
            poll.s2 = nullptr;
            if constexpr (std::is_same<T, float>::value)  // (the split engine keeps z in slot order only)
                if (use_cw2(p)) SG_TRY(cw2_launch_z_natural(c2tables(p, B), bf, s));
        }
        if (t % 4 == 3 && t + 2 < t_max - 1 && !tb.skip) SG_TRY(poll.request());
    }
    SG_TRY(pipe.join());
    SG_HIP(hipMemsetAsync(p->ws_argmax, 0x7f, sizeof(int32_t) * B * p->L, s));
    SG_TRY(reg_launch_map<T>(tb, bf, s));
    return copy_results(p, a, s);
}

template <typename T>
static int decode_impl(sg_amp_plan *p, const DecodeArgs &a, hipStream_t s) {
    const int B = a.B, t_max = a.t_max;
    SG_TRY(ensure_ws(p, B, t_max));
    if (p->regular) return decode_regular<T>(p, a, s);
    AmpTables<T> tb = tables<T>(p);
    AmpBufs<T> bf = bufs<T>(p, B, a.d_y);
    bf.true_idx = a.d_true;
    const AmpScalars sc = scalars(p);
    const AmpParams pr = params(p, a);
    const size_t rs = sizeof(T);
    SG_HIP(hipMemsetAsync(p->ws_beta, 0, (size_t)B * p->LM * rs, s));
    SG_TRY(amp_launch_control<T>(tb, bf, sc, pr, 2, 0, s));
    ActivePoll poll{p, B, s};
    const bool blk =(p->block || p->block2) && sizeof(T) == 4;
    const BlkTables bt = blk ? btables(p) : BlkTables{};
    p->last_engine = blk ? 3 : 0;
    p->last_handover = -1;
    for (int t = 0; t < t_max - 1; ++t) {
        if constexpr (sizeof(T) == 4) {
            if (blk) {
                // (both block engines run iteration t's Ab inside iteration t - 1's Az)
                SG_TRY(amp_launch_control<T>(tb, bf, sc, pr, 0, t, s));
                SG_TRY(p->block2 ? blk2_launch_az(bt, bf, (cx<float> *)p->ws_gbuf, t + 1 < t_max - 1, s)
                                 : blk_launch_az(bt, bf, t + 1 < t_max - 1, s));
                SG_TRY(amp_launch_control<T>(tb, bf, sc, pr, 1, t, s));
            }
        }
        if (!blk) {
            if (t > 0) SG_TRY(amp_launch_ab<T>(tb, bf, s));
            SG_TRY(amp_launch_control<T>(tb, bf, sc, pr, 0, t, s));
            SG_TRY(amp_launch_az<T>(tb, bf, s));
            SG_TRY(amp_launch_eta<T>(tb, bf, s));
            SG_TRY(amp_launch_control<T>(tb, bf, sc, pr, 1, t, s));
        }
        // skip the remaining launches once every codeword stopped (ActivePoll: the flags after
        // iterations 3, 7, 11, ..., read one iteration later)
        bool stopped = false;
        SG_TRY(poll.step(t % 4 == 3 && t + 2 < t_max - 1, &stopped));
        if (stopped) break;
    }
    return copy_results(p, a, s);
}

// The enqueue part of the design operators: in and out are device vectors of the plan precision in natural
// order (transpose 0: in [B][LM] -> out [B][n]; 1: in [B][n] -> out [B][LM]).  Launches only -- no stream
// synchronisation, no host-to-device copy -- in the workspace ensure_ws(p, B, 2) holds.  The general engine reads
// its input from ws_beta / ws_z (copied there unless it already is) and needs every codeword active and phi = 1
// on the device before (apply_impl uploads them, the integrated loop sets them once before its first iteration).
template <typename T>
static int apply_enqueue(sg_amp_plan *p, int transpose, const T *in, int B, T *out, hipStream_t s) {
    if (p->regular) {
        RegTables<T> rt = rtables<T>(p);
        RegBufs<T> rf = rbufs<T>(p, B, nullptr);
        rf.mode = 1;
        rf.ext_in = in;
        rf.ext_out = out;
        if (!transpose) {
            SG_TRY(reg_launch_ab<T>(rt, rf, s));
            SG_TRY(reg_launch_ab_finish<T>(rt, rf, s));
        } else {
            SG_TRY(reg_launch_az<T>(rt, rf, 0, s));
        }
        return SG_OK;
    }
    AmpTables<T> tb = tables<T>(p);
    AmpBufs<T> bf = bufs<T>(p, B, nullptr);
    if (!transpose) {
        if (in != (const T *)p->ws_beta)
            SG_HIP(hipMemcpyAsync(p->ws_beta, in, (size_t)B * p->LM * sizeof(T), hipMemcpyDeviceToDevice, s));
        SG_TRY(amp_launch_ab<T>(tb, bf, s));
        SG_TRY(amp_launch_rowsum<T>(tb, bf, out, s));
    } else {
        if (in != (const T *)p->ws_z)
            SG_HIP(hipMemcpyAsync(p->ws_z, in, (size_t)B * p->n * sizeof(T), hipMemcpyDeviceToDevice, s));
        SG_TRY(amp_launch_az<T>(tb, bf, s));
        SG_TRY(amp_launch_colgather<T>(tb, bf, out, s));
    }
    return SG_OK;
}

// A design operator on vectors of either type: cast into the workspace, enqueue, cast back.  Staged there: [B][LM]
// vectors in ws_s (regular plan) / ws_beta (general), Az's [B][n] input in ws_y / ws_z, Ab's [B][n] output in ws_z.
template <typename T>
static int apply_impl(sg_amp_plan *p, int transpose, const void *d_in, int in_is_double, int B, void *d_out,
                      int out_double, hipStream_t s) {
    SG_TRY(ensure_ws(p, B, 2));
    const size_t nin = (size_t)B * (transpose ? p->n : p->LM), nout = (size_t)B * (transpose ? p->LM : p->n);
    T *const vLM = (T *)(p->regular ? p->ws_s : p->ws_beta);
    T *const in = transpose ? (T *)(p->regular ? p->ws_y : p->ws_z) : vLM;
    T *const out = !out_double ? (T *)d_out : transpose ? vLM : (T *)p->ws_z;
    std::vector<int32_t> ones;  // the general engine's kernels read the active flags, Az also phi: all 1
    std::vector<double> ph;
    if (!p->regular) {
        ones.assign(B, 1);
        SG_HIP(hipMemcpyAsync(p->ws_active, ones.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    }
    SG_TRY(amp_launch_cast<T>(d_in, in_is_double, in, nin, s));
    if (!p->regular && transpose) {
        ph.assign((size_t)B * p->Lr, 1.0);
        SG_HIP(hipMemcpyAsync(p->ws_phi, ph.data(), sizeof(double) * ph.size(), hipMemcpyHostToDevice, s));
    }
    SG_TRY(apply_enqueue<T>(p, transpose, in, B, out, s));
    if (out_double) SG_TRY(amp_launch_uncast<T>(out, (double *)d_out, nout, s));
    SG_HIP(hipStreamSynchronize(s));
    return SG_OK;
}

// The front end of integ_loop (integ_loop.hpp) on a flat plan: the plan's operators on natural-order vectors, and
// one section kernel (integrated_dct.hip) for the dense front end's three passes eta / bit probabilities / LLRs.
// beta lives in the plan's [B][LM] workspace (ws_s of a regular plan, ws_beta of a general one), z in ws_z, tau^2
// in the plan's tau slot ([B], Lc = 1); u = Az(z) is written into the alpha buffer, where the section kernel turns
// it into the weighted alpha.
template <typename T>
struct DctFront {
    sg_amp_plan *p;
    int B, t_max;
    const T *y;
    double *tau_hist;  // [B][t_max] or null
    double P, snp;
    DenseBufs<T> db;  // dense_launch_bsq reads beta, the shape and sec_bsq only
    T *beta() const { return db.beta; }
    const double *tau() const { return p->ws_tau; }
    const DenseBufs<T> &bsq_view() const { return db; }
    int forward(hipStream_t s) { return apply_enqueue<T>(p, 0, db.beta, B, (T *)p->wi.x, s); }  // Ab(beta) = snp A beta
    int residual(int t, int ons_mode, hipStream_t s) {  // (the kernel writes the history itself)
        return idct_launch_residual<T>(y, (const T *)p->wi.x, (T *)p->ws_z, B, p->n, p->L, snp, P, ons_mode, p->wi.ons,
                                       p->wi.part, t, p->ws_tau, tau_hist, t_max, s);
    }
    int sections(int, hipStream_t s) {
        SG_TRY(apply_enqueue<T>(p, 1, (const T *)p->ws_z, B, (T *)p->wi.alpha, s));  // u = Az(z) = snp A^T z
        return idct_launch_section<T>((T *)p->wi.alpha, db.beta, p->ws_tau, B, p->L, p->M, snp, (T *)p->wi.vk0,
                                      (T *)p->wi.llr, s);
    }
    // 1 / (1 + e^-app), finite for every app: this loop's single-precision LLRs pass the e^app overflow
    int probs(const T *app, size_t nn, T *vk, hipStream_t s) { return idct_launch_probs<T>(app, nn, vk, s); }
};

template <typename T>
static int integ_dct_impl(sg_amp_plan *p, sg_graph *g, int mode, int N, int K, const void *d_y, int B, int t_max,
                          int its, int its_final, uint8_t *d_bits, void *d_app, double *d_tau_hist, hipStream_t s) {
    SG_TRY(ensure_ws(p, B, 2));
    SG_TRY(p->wi.ensure(B, p->L, p->LM, p->n, p->L * ilog2(p->M), sizeof(T), true));
    const double P = p->W[0];
    DctFront<T> front{p, B, t_max, (const T *)d_y, d_tau_hist, P, std::sqrt((double)p->n * (P / p->L)), {}};
    DenseBufs<T> &db = front.db;
    db.L = p->L; db.M = p->M; db.LM = p->LM; db.B = B; db.sec_bsq = p->wi.part;
    db.beta = p->regular ? (T *)p->ws_s : (T *)p->ws_beta;
    SG_HIP(hipMemsetAsync(front.beta(), 0, (size_t)B * p->LM * sizeof(T), s));
    if (!p->regular) SG_TRY(idct_launch_ones(p->ws_active, B, p->ws_phi, B * p->Lr, s));
    return integ_loop<T>(front, p->wi, g, mode, N, K, B, p->L, p->M, t_max, its, its_final, d_bits, d_app, s);
}

// The operator-loop decoder (amp_oploop.hip), for AMP with known sections (rule Known, d_known given) and real
// K = 2 modulated AMP (rule Bpsk; a.d_true then holds words, and so does d_known: null for the plain decode, given
// for the decode with known words, which keeps no soft state): sparc_amp with the plan's operators on
// natural-order vectors, as integ_dct_impl runs them.  beta lives in the plan's [B][LM] workspace (ws_s of a
// regular plan, ws_beta of a general one) and z / phi in ws_z, where apply_enqueue reads them without a copy; z,
// r = Ab(beta), u = Az(z / phi), the sums of z^2 per row block and the section sums in the loop's own buffers
// (wp); the per-codeword scalars and results in the batch workspace's slots, so copy_results ends the call.  phi,
// gamma and b are per row block (W of ndim 2; phi in ws_phi_prev: the general engine's Az divides by ws_phi, which
// stays 1).  Nothing but launches inside the loop; the loop's own active flags are polled like a decode's.
template <typename T>
static int oploop_impl(sg_amp_plan *p, const DecodeArgs &a, SectionRule rule, const int32_t *d_known, hipStream_t s) {
    const int B = a.B, t_max = a.t_max;
    SG_TRY(ensure_ws(p, B, t_max));
    SG_TRY(partial_ensure_ws(p, B));
    OpLoopBufs<T> ob{};
    ob.B = B; ob.L = p->L; ob.M = p->M; ob.LM = p->LM; ob.n = p->n; ob.Lr = p->Lr; ob.Lc = p->Lc; ob.Mr = p->Mr;
    ob.ndim = p->ndim; ob.t_max = t_max; ob.np = part_count(p->Mr);
    ob.y = (const T *)a.d_y;
    ob.beta = p->regular ? (T *)p->ws_s : (T *)p->ws_beta;
    ob.u = (T *)p->wp_u; ob.r = (T *)p->wp_r; ob.z = (T *)p->wp_z; ob.zs = (T *)p->ws_z;
    ob.known = d_known; ob.truth = a.d_true;
    if (rule == SectionRule::Bpsk && !d_known && p->bpsk_soft) ob.s_keep = (T *)p->wp_skeep;  // (partial_ensure_ws)
    ob.zz = p->wp_zz; ob.bsq = p->wp_bsq; ob.err = p->wp_err; ob.map = p->ws_argmax;
    ob.psi = p->ws_psi; ob.psi_prev = p->ws_psi_prev; ob.gamma = p->ws_gamma; ob.bco = p->ws_bco;
    ob.phi = p->ws_phi_prev; ob.tau = p->wp_tau; ob.nmse = p->ws_nmse;
    ob.active = p->wp_active; ob.t_final = p->ws_tfinal;
    ob.W = p->dW; ob.awgn_var = a.awgn_var; ob.rtol = a.rtol;
    ob.atol = 2e-15;  // 2*np.finfo(float).resolution, sparc.py:916
    ob.phi_method = a.phi_method;
    SG_HIP(hipMemsetAsync(ob.beta, 0, (size_t)B * p->LM * sizeof(T), s));
    if (!p->regular) SG_TRY(idct_launch_ones(p->ws_active, B, p->ws_phi, B * p->Lr, s));
    SG_TRY(oploop_launch_init<T>(ob, rule, s));
    ActivePoll poll{p, B, s, false, p->wp_active};
    for (int t = 0; t < t_max - 1; ++t) {
        SG_TRY(apply_enqueue<T>(p, 0, ob.beta, B, ob.r, s));  // r = Ab(beta) (t = 0: of the known one-hots, or of zero)
        SG_TRY(oploop_launch_residual<T>(ob, t, s));
        SG_TRY(oploop_launch_control<T>(ob, 0, t, s));
        SG_TRY(apply_enqueue<T>(p, 1, ob.zs, B, ob.u, s));  // u = Az(z / phi)
        SG_TRY(oploop_launch_section<T>(ob, rule, s));
        SG_TRY(oploop_launch_control<T>(ob, 1, t, s));
        // skip the remaining launches once every codeword stopped (ActivePoll: the flags after iterations 3, 7,
        // 11, ..., read one iteration later)
        bool stopped = false;
        SG_TRY(poll.step(t % 4 == 3 && t + 2 < t_max - 1, &stopped));
        if (stopped) break;
    }
    return copy_results(p, a, s);
}

// The refusals of a decode's scalar parameters
static int param_checks(double awgn_var, int t_max, double rtol, int phi_method) {
    SG_CHECK_ARG(t_max > 1, "t_max must be > 1 (sparc.py:168)");
    SG_CHECK_ARG(rtol > 0 && rtol < 1, "rtol must be in (0, 1)");
    SG_CHECK_ARG(phi_method == 1 || phi_method == 2, "phi_est_method must be 1 or 2");
    SG_CHECK_ARG(awgn_var >= 0, "awgn_var must be >= 0");
    return SG_OK;
}

// Every refusal of an operator-loop decode that needs no device (header, sg_amp_decode_partial_device,
// sg_amp_decode_bpsk_device and sg_amp_decode_bpsk_partial_device).  The K = 2 rule takes a spatially coupled W
// with and without known words (held against tests/bpsk_partial_ref.py); the unmodulated rule with known sections
// has no reference on such a W, so that stays refused.
static int oploop_checks(const sg_amp_plan *p, SectionRule rule, double awgn_var, int t_max, double rtol,
                         int phi_method) {
    if (rule == SectionRule::Known && p->ndim == 2)
        return fail(SG_ERR_UNSUPPORTED, "AMP with known sections takes a flat or power-allocated design (W of ndim 0 "
                    "or 1), not a spatially coupled one");
    if (p->M < 2 || (p->M & (p->M - 1)) != 0 || p->M > 2048)
        return fail(SG_ERR_UNSUPPORTED, "section size M = %d: the %s section kernel takes a power of two in "
                    "[2, 2048]", p->M, rule_name(rule));
    return param_checks(awgn_var, t_max, rtol, phi_method);
}

// The host side of a decode, after the entry point's refusals: y (and the known and true sections) into the plan's
// buffers, the decode there, the results back.  No rule: decode_impl; a rule: oploop_impl with it (for Bpsk
// known_idx, true_idx and map_idx hold section words, and known_idx may be null).
static int decode_host(sg_amp_plan *p, const double *y, int B, std::optional<SectionRule> rule,
                       const int32_t *known_idx, const int32_t *true_idx, double awgn_var, int t_max, double rtol,
                       int phi_method, int32_t *map_idx, int32_t *t_final, double *nmse, double *psi) {
    SG_HIP(hipSetDevice(p->device));
    hipStream_t s = lib_stream();
    // (the workspace before the staging buffer: growing the workspace frees io too)
    SG_TRY(ensure_ws(p, B, t_max));
    if (rule) SG_TRY(partial_ensure_ws(p, B));
    const size_t ny = (size_t)B * p->n, nsec = (size_t)B * p->L;
    SG_TRY(ensure_io(p, ny * sizeof(double)));
    SG_HIP(hipMemcpyAsync(p->io.at(), y, ny * sizeof(double), hipMemcpyHostToDevice, s));
    if (known_idx) SG_HIP(hipMemcpyAsync(p->wp_known, known_idx, sizeof(int32_t) * nsec, hipMemcpyHostToDevice, s));
    if (true_idx) SG_HIP(hipMemcpyAsync(p->ws_true, true_idx, sizeof(int32_t) * nsec, hipMemcpyHostToDevice, s));
    SG_TRY(by_precision(p->precision, [&](auto t) {
        using T = decltype(t);
        SG_TRY(amp_launch_cast<T>(p->io.at(), 1, (T *)p->ws_y, ny, s));
        const DecodeArgs a{p->ws_y, B, true_idx ? p->ws_true : nullptr, awgn_var, t_max, rtol, phi_method,
                           nullptr, nullptr, nullptr, nullptr};
        if (!rule) return decode_impl<T>(p, a, s);
        return oploop_impl<T>(p, a, *rule, known_idx ? p->wp_known : nullptr, s);
    }));
    SG_HIP(hipMemcpyAsync(map_idx, p->ws_argmax, sizeof(int32_t) * nsec, hipMemcpyDeviceToHost, s));
    SG_HIP(hipMemcpyAsync(t_final, p->ws_tfinal, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
    SG_HIP(hipMemcpyAsync(nmse, p->ws_nmse, sizeof(double) * B * t_max * p->Lc, hipMemcpyDeviceToHost, s));
    SG_HIP(hipMemcpyAsync(psi, p->ws_psi, sizeof(double) * B * p->Lc, hipMemcpyDeviceToHost, s));
    SG_HIP(hipStreamSynchronize(s));
    return SG_OK;
}

}  // namespace sg

using namespace sg;

// One-hot message vectors (value 1, the public SPARC's beta0 before the
// sqrt(W / L) scaling that the design applies, sparc.py:17-53) -> x = A beta0.
template <typename T>
__global__ void onehot_one_kernel(const int32_t *idx, int L, int M, T *beta) {
    const int b = blockIdx.y;
    for (int l = blockIdx.x * blockDim.x + threadIdx.x; l < L; l += gridDim.x * blockDim.x)
        beta[(size_t)b * L * M + (size_t)l * M + idx[(size_t)b * L + l]] = T(1);
}

// K = 2: section words (location << 1) | symbol -> beta0 with +1 (symbol 0) or -1 at the location; a word outside
// [0, 2M) leaves its section zero.
template <typename T>
__global__ void onehot_bpsk_kernel(const int32_t *word, int L, int M, T *beta) {
    const int b = blockIdx.y;
    for (int l = blockIdx.x * blockDim.x + threadIdx.x; l < L; l += gridDim.x * blockDim.x) {
        const int w = word[(size_t)b * L + l];
        if (w >= 0 && w < 2 * M) beta[(size_t)b * L * M + (size_t)l * M + (w >> 1)] = (w & 1) ? T(-1) : T(1);
    }
}

template <typename T>
static int encode_impl(sg_amp_plan *p, const int32_t *d_idx, int B, T *d_x, hipStream_t s, bool bpsk = false) {
    SG_TRY(ensure_ws(p, B, 2));
    T *beta0 = p->regular ? (T *)p->ws_s : (T *)p->ws_beta;  // (where apply_enqueue reads it without a copy)
    SG_HIP(hipMemsetAsync(beta0, 0, (size_t)B * p->LM * sizeof(T), s));
    const dim3 grid((p->L + 255) / 256, B);
    if (bpsk) hipLaunchKernelGGL(onehot_bpsk_kernel<T>, grid, dim3(256), 0, s, d_idx, p->L, p->M, beta0);
    else hipLaunchKernelGGL(onehot_one_kernel<T>, grid, dim3(256), 0, s, d_idx, p->L, p->M, beta0);
    std::vector<int32_t> ones;
    if (!p->regular) {  // the general engine: all codewords active
        ones.assign(B, 1);
        SG_HIP(hipMemcpyAsync(p->ws_active, ones.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    }
    SG_TRY(apply_enqueue<T>(p, 0, beta0, B, d_x, s));
    if (!p->regular) SG_HIP(hipStreamSynchronize(s));  // the host vector above
    return SG_OK;
}

// sg_amp_last_decode reports what the latest decode call ran: reset at the
// entry of every decode, so a call that returns early (B == 0) or fails
// partway reports engine -1 instead of a previous call's engine and hand-over
static void reset_last(sg_amp_plan *p) {
    for (sg_amp_plan *q : {p, p->alt}) {
        if (!q) continue;
        q->last_ran = nullptr;
        q->last_engine = -1;
        q->last_handover = -1;
        q->last_piped = 0;
        q->last_B = 0;
        q->last_bpsk_B = 0;
    }
}

// What the six entry points of the operator-loop decoder share: every refusal that needs no buffer, then `body`
// on the call's stream (the host variants go on through decode_host, on the library's).  The call clears the
// last-decode state: the loop runs in the workspace that holds a decode's final state.  keeps_soft: a plain K = 2
// decode (nothing known), the only one that fills s_keep.
template <typename Body>
static int oploop_entry(sg_amp_plan *p, SectionRule rule, bool keeps_soft, int B, double awgn_var, int t_max,
                        double rtol, int phi_method, void *stream, Body &&body) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p, "plan is NULL");
    reset_last(p);
    SG_TRY(oploop_checks(p, rule, awgn_var, t_max, rtol, phi_method));
    if (B <= 0) return SG_OK;
    SG_HIP(hipSetDevice(p->device));
    SG_TRY(body(pick_stream(stream)));
    if (keeps_soft && p->bpsk_soft) p->last_bpsk_B = B;  // s_keep and wp_tau hold its final state
    return SG_OK;
}

extern "C" {

int sg_amp_plan_engine(const sg_amp_plan *p, int B) {
    SG_CHECK_ARG(p, "plan is NULL");
    if (p->regular) return (sg::use_cw(p, B) && (p->precision == SG_F32 || sg::use_cw2(p))) ? 2 : 1;
    return (p->block || p->block2) ? 3 : 0;
}

int sg_amp_plan_set_cus(sg_amp_plan *p, int cus) {
    SG_CHECK_ARG(p && cus >= 0, "plan is NULL or negative CU count");
    for (sg_amp_plan *q : {p, p->alt})
        if (q) q->cus_assumed = cus;
    return SG_OK;
}

int sg_amp_last_pipelined(const sg_amp_plan *p, int *pipelined) {
    SG_CHECK_ARG(p && pipelined, "null argument");
    const sg_amp_plan *r = p->last_ran ? p->last_ran : p;
    *pipelined = r->last_piped;
    return SG_OK;
}

int sg_amp_last_decode(const sg_amp_plan *p, int *engine, int *handover_iter, int *on_companion) {
    SG_CHECK_ARG(p && engine && handover_iter, "null argument");
    const sg_amp_plan *r = p->last_ran ? p->last_ran : p;
    *engine = r->last_engine;
    *handover_iter = r->last_handover;
    if (on_companion) *on_companion = (p->last_ran && p->last_ran != p) ? 1 : 0;
    return SG_OK;
}

int sg_amp_decode_device(sg_amp_plan *p, const void *d_y, int B, const int32_t *d_true_idx, double awgn_var,
                         int t_max, double rtol, int phi_method, int32_t *d_map_idx, int32_t *d_t_final,
                         double *d_nmse, double *d_psi, void *stream) {
    SG_CHECK_ARG(p, "plan is NULL");
    reset_last(p);
    SG_TRY(sg::param_checks(awgn_var, t_max, rtol, phi_method));
    SG_CHECK_ARG(B >= 0, "negative batch");
    if (B == 0) return SG_OK;
    SG_CHECK_ARG(d_y, "d_y is NULL");
    sg_amp_plan *const handle = p;
    p = p->last_ran = sg::decode_plan(p, B);
    SG_TRY(ensure_device());
    SG_HIP(hipSetDevice(p->device));
    hipStream_t s = pick_stream(stream);
    const DecodeArgs a{d_y, B, d_true_idx, awgn_var, t_max, rtol, phi_method, d_map_idx, d_t_final, d_nmse, d_psi};
    SG_TRY(by_precision(p->precision, [&](auto t) { return decode_impl<decltype(t)>(p, a, s); }));
    handle->last_B = B;
    return SG_OK;
}

int sg_amp_decode(sg_amp_plan *p, const double *y, int B, const int32_t *true_idx, double awgn_var, int t_max,
                  double rtol, int phi_method, int32_t *map_idx, int32_t *t_final, double *nmse, double *psi) {
    SG_CHECK_ARG(p, "plan is NULL");
    reset_last(p);
    SG_CHECK_ARG(B >= 0, "negative batch");
    if (B == 0) return SG_OK;
    SG_CHECK_ARG(y && map_idx && t_final && nmse && psi, "null host buffer");
    SG_CHECK_ARG(t_max > 1, "t_max must be > 1 (sparc.py:168)");
    sg_amp_plan *const handle = p;
    p = p->last_ran = sg::decode_plan(p, B);
    SG_TRY(ensure_device());
    SG_TRY(sg::decode_host(p, y, B, std::nullopt, nullptr, true_idx, awgn_var, t_max, rtol, phi_method, map_idx,
                           t_final, nmse, psi));
    handle->last_B = B;
    return SG_OK;
}

int sg_amp_decode_partial_device(sg_amp_plan *p, const void *d_y, int B, const int32_t *d_known_idx,
                                 const int32_t *d_true_idx, double awgn_var, int t_max, double rtol, int phi_method,
                                 int32_t *d_map_idx, int32_t *d_t_final, double *d_nmse, double *d_psi, void *stream) {
    return oploop_entry(p, SectionRule::Known, false, B, awgn_var, t_max, rtol, phi_method, stream, [&](hipStream_t s) {
        SG_CHECK_ARG(d_y && d_known_idx, "d_y or d_known_idx is NULL");
        const DecodeArgs a{d_y, B, d_true_idx, awgn_var, t_max, rtol, phi_method, d_map_idx, d_t_final, d_nmse, d_psi};
        return by_precision(p->precision, [&](auto t) {
            return oploop_impl<decltype(t)>(p, a, SectionRule::Known, d_known_idx, s);
        });
    });
}

int sg_amp_decode_partial(sg_amp_plan *p, const double *y, int B, const int32_t *known_idx, const int32_t *true_idx,
                          double awgn_var, int t_max, double rtol, int phi_method, int32_t *map_idx, int32_t *t_final,
                          double *nmse, double *psi) {
    return oploop_entry(p, SectionRule::Known, false, B, awgn_var, t_max, rtol, phi_method, nullptr, [&](hipStream_t) {
        SG_CHECK_ARG(y && known_idx && map_idx && t_final && nmse && psi, "null host buffer");
        for (size_t i = 0; i < (size_t)B * p->L; ++i)
            SG_CHECK_ARG(known_idx[i] >= -1 && known_idx[i] < p->M, "known_idx[%zu] = %d outside [-1, %d)", i,
                         (int)known_idx[i], p->M);
        return sg::decode_host(p, y, B, SectionRule::Known, known_idx, true_idx, awgn_var, t_max, rtol, phi_method,
                               map_idx, t_final, nmse, psi);
    });
}

int sg_amp_decode_bpsk_device(sg_amp_plan *p, const void *d_y, int B, const int32_t *d_true_word, double awgn_var,
                              int t_max, double rtol, int phi_method, int32_t *d_map_word, int32_t *d_t_final,
                              double *d_nmse, double *d_psi, void *stream) {
    return oploop_entry(p, SectionRule::Bpsk, true, B, awgn_var, t_max, rtol, phi_method, stream, [&](hipStream_t s) {
        SG_CHECK_ARG(d_y, "d_y is NULL");
        const DecodeArgs a{d_y, B, d_true_word, awgn_var, t_max, rtol, phi_method, d_map_word, d_t_final, d_nmse,
                           d_psi};
        return by_precision(p->precision, [&](auto t) {
            return oploop_impl<decltype(t)>(p, a, SectionRule::Bpsk, nullptr, s);
        });
    });
}

int sg_amp_decode_bpsk(sg_amp_plan *p, const double *y, int B, const int32_t *true_word, double awgn_var, int t_max,
                       double rtol, int phi_method, int32_t *map_word, int32_t *t_final, double *nmse, double *psi) {
    return oploop_entry(p, SectionRule::Bpsk, true, B, awgn_var, t_max, rtol, phi_method, nullptr, [&](hipStream_t) {
        SG_CHECK_ARG(y && map_word && t_final && nmse && psi, "null host buffer");
        return sg::decode_host(p, y, B, SectionRule::Bpsk, nullptr, true_word, awgn_var, t_max, rtol, phi_method,
                               map_word, t_final, nmse, psi);
    });
}

int sg_amp_decode_bpsk_partial_device(sg_amp_plan *p, const void *d_y, int B, const int32_t *d_known_word,
                                      const int32_t *d_true_word, double awgn_var, int t_max, double rtol,
                                      int phi_method, int32_t *d_map_word, int32_t *d_t_final, double *d_nmse,
                                      double *d_psi, void *stream) {
    return oploop_entry(p, SectionRule::Bpsk, false, B, awgn_var, t_max, rtol, phi_method, stream, [&](hipStream_t s) {
        SG_CHECK_ARG(d_y && d_known_word, "d_y or d_known_word is NULL");
        const DecodeArgs a{d_y, B, d_true_word, awgn_var, t_max, rtol, phi_method, d_map_word, d_t_final, d_nmse,
                           d_psi};
        return by_precision(p->precision, [&](auto t) {
            return oploop_impl<decltype(t)>(p, a, SectionRule::Bpsk, d_known_word, s);
        });
    });
}

int sg_amp_decode_bpsk_partial(sg_amp_plan *p, const double *y, int B, const int32_t *known_word,
                               const int32_t *true_word, double awgn_var, int t_max, double rtol, int phi_method,
                               int32_t *map_word, int32_t *t_final, double *nmse, double *psi) {
    return oploop_entry(p, SectionRule::Bpsk, false, B, awgn_var, t_max, rtol, phi_method, nullptr, [&](hipStream_t) {
        SG_CHECK_ARG(y && known_word && map_word && t_final && nmse && psi, "null host buffer");
        for (size_t i = 0; i < (size_t)B * p->L; ++i)
            SG_CHECK_ARG(known_word[i] >= -1 && known_word[i] < 2 * p->M, "known_word[%zu] = %d outside [-1, %d)", i,
                         (int)known_word[i], 2 * p->M);
        return sg::decode_host(p, y, B, SectionRule::Bpsk, known_word, true_word, awgn_var, t_max, rtol, phi_method,
                               map_word, t_final, nmse, psi);
    });
}

int sg_concat_known_sections_device(int precision, const void *d_app, const int32_t *d_it, int max_it, int B, int mults,
                                    int N, int L, int L_unprotected, int logM, int32_t *d_known_idx, void *stream) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(d_app && d_it && d_known_idx, "null device buffer");
    SG_CHECK_ARG(L > 0 && L_unprotected >= 0 && L_unprotected <= L && logM >= 1 && logM <= 30 && N > 0 && mults >= 0,
                 "bad lengths");
    SG_CHECK_ARG((long long)(L - L_unprotected) * logM <= (long long)mults * N,
                 "%d protected sections of %d bits do not fit %d blocks of %d bits", L - L_unprotected, logM, mults, N);
    if (B <= 0) return SG_OK;
    hipStream_t s = pick_stream(stream);
    return by_precision(precision, [&](auto t) {
        return part_launch_known((const decltype(t) *)d_app, d_it, max_it, B, mults, N, L, L_unprotected, logM,
                                 d_known_idx, s);
    });
}

int sg_amp_apply(sg_amp_plan *p, int transpose, const double *in, int B, double *out) {
    SG_CHECK_ARG(p && in && out, "null argument");
    SG_CHECK_ARG(B >= 0, "negative batch");
    if (B == 0) return SG_OK;
    p->last_B = p->last_bpsk_B = 0;  // (the operators run in the workspace that holds a decode's final state)
    SG_TRY(ensure_device());
    SG_HIP(hipSetDevice(p->device));
    hipStream_t s = lib_stream();
    const size_t nin = (size_t)B * (transpose ? p->n : p->LM), nout = (size_t)B * (transpose ? p->LM : p->n);
    SG_TRY(ensure_ws(p, B, 2));
    SG_TRY(ensure_io(p, (nin + nout) * sizeof(double)));
    double *din = p->io.at<double>(), *dout = din + nin;
    SG_HIP(hipMemcpyAsync(din, in, nin * sizeof(double), hipMemcpyHostToDevice, s));
    SG_TRY(by_precision(p->precision,
                        [&](auto t) { return apply_impl<decltype(t)>(p, transpose, din, 1, B, dout, 1, s); }));
    SG_HIP(hipMemcpyAsync(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost, s));
    SG_HIP(hipStreamSynchronize(s));
    return SG_OK;
}

int sg_amp_encode_device(sg_amp_plan *p, const int32_t *d_idx, int B, void *d_x, void *stream) {
    SG_CHECK_ARG(p && d_idx && d_x, "null argument");
    if (B <= 0) return SG_OK;
    p->last_B = p->last_bpsk_B = 0;
    SG_TRY(ensure_device());
    hipStream_t s = pick_stream(stream);
    return by_precision(p->precision, [&](auto t) { return encode_impl(p, d_idx, B, (decltype(t) *)d_x, s); });
}

int sg_amp_encode_bpsk_device(sg_amp_plan *p, const int32_t *d_word, int B, void *d_x, void *stream) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p && d_word && d_x, "null argument");
    if (B <= 0) return SG_OK;
    p->last_B = p->last_bpsk_B = 0;
    hipStream_t s = pick_stream(stream);
    return by_precision(p->precision, [&](auto t) { return encode_impl(p, d_word, B, (decltype(t) *)d_x, s, true); });
}

// Diagnostics: mean shader-clock cycles between the phase timestamps of the
// last stage-1 launches (kernel 0 = reg_ab_stage1, 1 = reg_az_stage2), over
// every workgroup that recorded them; needs SG_AMP_TPROF set at plan use.
int sg_amp_stage_profile(sg_amp_plan *p, int kernel, double *mean_cycles, int *nphases) {
    SG_CHECK_ARG(p && mean_cycles && nphases && (kernel == 0 || kernel == 1), "bad argument");
    *nphases = 0;
    if (p->last_ran) p = p->last_ran;  // the sub-plan the last decode ran on (maybe the companion)
    const uint64_t *tp = p->tprof.at<uint64_t>();
    if (!tp) return SG_OK;
    std::vector<uint64_t> h(p->tprof_items * 8);
    SG_HIP(hipDeviceSynchronize());
    SG_HIP(hipMemcpy(h.data(), tp + (size_t)kernel * p->tprof_items * 8, h.size() * 8, hipMemcpyDeviceToHost));
    double sum[8] = {0};
    size_t n = 0;
    for (size_t i = 0; i < p->tprof_items; ++i) {
        const uint64_t *r = &h[i * 8];
        if (!r[0] || !r[7]) continue;
        ++n;
        for (int k = 1; k < 8; ++k) sum[k] += (double)(r[k] - r[k - 1]);
    }
    for (int k = 0; k < 8; ++k) mean_cycles[k] = n ? sum[k] / n : 0.0;
    *nphases = 8;
    return SG_OK;
}

int sg_amp_stage_raw(sg_amp_plan *p, int kernel, uint64_t *out, size_t *items) {
    SG_CHECK_ARG(p && items && (kernel == 0 || kernel == 1), "bad argument");
    if (p->last_ran) p = p->last_ran;
    const uint64_t *tp = p->tprof.at<uint64_t>();
    *items = tp ? p->tprof_items : 0;
    if (!tp || !out) return SG_OK;
    const size_t ni = p->tprof_items;
    std::vector<uint64_t> cyc(ni * 8), rt(ni * 2);
    SG_HIP(hipDeviceSynchronize());
    SG_HIP(hipMemcpy(cyc.data(), tp + (size_t)kernel * ni * 8, ni * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    SG_HIP(hipMemcpy(rt.data(), tp + ni * 16 + (size_t)kernel * ni * 2, ni * 2 * sizeof(uint64_t),
                     hipMemcpyDeviceToHost));
    for (size_t i = 0; i < ni; ++i) {
        std::copy(&cyc[i * 8], &cyc[i * 8] + 8, out + i * 10);
        out[i * 10 + 8] = rt[i * 2];
        out[i * 10 + 9] = rt[i * 2 + 1];
    }
    return SG_OK;
}

int sg_amp_apply_device(sg_amp_plan *p, int transpose, const void *d_in, int B, void *d_out, void *stream) {
    SG_CHECK_ARG(p && d_in && d_out, "null argument");
    if (B <= 0) return SG_OK;
    p->last_B = p->last_bpsk_B = 0;
    SG_TRY(ensure_device());
    hipStream_t s = pick_stream(stream);
    return by_precision(p->precision, [&](auto t) {  // (vectors of the plan precision on both sides)
        return apply_impl<decltype(t)>(p, transpose, d_in, sizeof(t) == 8, B, d_out, 0, s);
    });
}

}  // extern "C"

// Soft output of the last decode.  Final-state contract of the engines (DESIGN.md "Soft output of the DCT
// engines"): every regular engine -- staged, per-codeword, split f32 / f64, with or without a hand-over -- leaves
// s in class order in ws_s (reg_launch_map reads it there) and, per codeword, the tau of the iteration that wrote
// that s in ws_tau: their kernels return at once for a stopped codeword, so later iterations of the others move
// neither (ws_tau_prev is the iteration before).  The general engine leaves beta in natural order in ws_beta.
static int llr_checks(sg_amp_plan *p, int B, int l0, int nl, int llr_ld, int *logM_out) {
    if ((p->block || p->block2) && p->precision == SG_F32)
        return fail(SG_ERR_UNSUPPORTED, "no soft output from the single-precision block engine (%s): decode the "
                    "spatially coupled design in double precision", p->block2 ? "amp_block2.hip" : "amp_block.hip");
    SG_CHECK_ARG(p->M >= 2 && (p->M & (p->M - 1)) == 0, "section size M = %d must be a power of two >= 2", p->M);
    SG_CHECK_ARG(p->last_ran && p->last_B > 0, "no decode through this plan yet (or its state was overwritten)");
    SG_CHECK_ARG(B == p->last_B, "B = %d, but the last decode held %d codewords", B, p->last_B);
    *logM_out = ilog2(p->M);
    return section_range_check(p->L, l0, nl, llr_ld, *logM_out, "log2 M");
}

// The host variants: launch(d_llr, stream) fills [B][ld] values of the plan's real type on the device (nv = B ld in
// all); out gets them as doubles.  Staging in io's own I/O buffer (not part of the decode state): doubles, then the
// plan's reals.
template <typename F>
static int llr_to_host(sg_amp_plan *io, int device, int precision, size_t nv, double *out, F &&launch) {
    if (nv == 0) return SG_OK;
    SG_HIP(hipSetDevice(device));
    hipStream_t s = lib_stream();
    SG_TRY(ensure_io(io, nv * 16));
    double *dd = io->io.at<double>();
    if (precision == SG_F64) {
        SG_TRY(launch(dd, s));
    } else {
        float *df = (float *)(dd + nv);
        SG_TRY(launch(df, s));
        SG_TRY(amp_launch_uncast<float>(df, dd, nv, s));
    }
    SG_HIP(hipMemcpyAsync(out, dd, nv * sizeof(double), hipMemcpyDeviceToHost, s));
    SG_HIP(hipStreamSynchronize(s));
    return SG_OK;
}

template <typename T>
static int llr_impl(const sg_amp_plan *r, int B, int l0, int nl, int llr_ld, int probs_only, T *d_llr, hipStream_t s) {
    if (r->regular)
        return reg_launch_llr<T>(rtables<T>(r), (const T *)r->ws_s, r->ws_tau, B, l0, nl, llr_ld, probs_only, d_llr, s);
    return glue_launch_llr<T>((const T *)r->ws_beta, B, r->L, r->M, l0, nl, 1.0, llr_ld, d_llr, probs_only, 1, s);
}

extern "C" {

int sg_amp_llr_device(sg_amp_plan *p, int B, int l0, int nl, int llr_ld, int probs_only, void *d_llr, void *stream) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p && d_llr, "null argument");
    int logM = 0;
    SG_TRY(llr_checks(p, B, l0, nl, llr_ld, &logM));
    const sg_amp_plan *r = p->last_ran;
    SG_HIP(hipSetDevice(r->device));
    hipStream_t s = pick_stream(stream);
    return by_precision(r->precision, [&](auto t) {
        return llr_impl(r, B, l0, nl, llr_ld, probs_only, (decltype(t) *)d_llr, s);
    });
}

int sg_amp_llr(sg_amp_plan *p, int B, int l0, int nl, int probs_only, double *out) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p && out, "null argument");
    int logM = 0;
    SG_TRY(llr_checks(p, B, l0, nl, INT32_MAX, &logM));
    const sg_amp_plan *r = p->last_ran;
    const int ld = nl * logM;  // (<= INT32_MAX: checked)
    return llr_to_host(p, r->device, r->precision, (size_t)B * ld, out, [&](auto *d, hipStream_t s) {
        return llr_impl(r, B, l0, nl, ld, probs_only, d, s);
    });
}

}  // extern "C"

// Soft output of the last K = 2 decode (amp_bpsk_llr.hip).  Final-state contract of the operator loop (DESIGN.md
// "Soft output of the K = 2 decoder"): the section and control kernels return at once for a stopped codeword, so
// wp_skeep and wp_tau hold, per codeword, the s and the tau of its last executed iteration.
static int bpsk_llr_checks(const sg_amp_plan *p, int B, int l0, int nl, long long llr_ld, int *per_out) {
    if (p->M < 2 || (p->M & (p->M - 1)) != 0 || p->M > 2048)
        return fail(SG_ERR_UNSUPPORTED, "section size M = %d: the K = 2 soft output takes a power of two in "
                    "[2, 2048]", p->M);
    SG_CHECK_ARG(p->bpsk_soft, "soft output is off: sg_amp_bpsk_soft_output(plan, 1) before the decode");
    SG_CHECK_ARG(p->last_bpsk_B > 0 && p->wp_skeep, "no K = 2 decode with soft output through this plan yet (or its "
                 "state was overwritten)");
    SG_CHECK_ARG(B == p->last_bpsk_B, "B = %d, but the last K = 2 decode held %d codewords", B, p->last_bpsk_B);
    *per_out = ilog2(p->M) + 1;
    return section_range_check(p->L, l0, nl, llr_ld, *per_out, "(log2 M + 1)");
}

template <typename T>
static int bpsk_llr_impl(const sg_amp_plan *p, int B, int l0, int nl, int llr_ld, int probs_only, T *d_llr,
                         hipStream_t s) {
    return bpsk_launch_llr<T>((const T *)p->wp_skeep, p->wp_tau, B, p->L, p->M, p->Lc, l0, nl, llr_ld, probs_only,
                              d_llr, s);
}

extern "C" {

int sg_amp_bpsk_soft_output(sg_amp_plan *p, int on) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p, "plan is NULL");
    p->bpsk_soft = on != 0;
    p->last_bpsk_B = 0;  // s_keep is filled by the next K = 2 decode
    return SG_OK;
}

int sg_amp_bpsk_llr_device(sg_amp_plan *p, int B, int l0, int nl, int llr_ld, int probs_only, void *d_llr,
                           void *stream) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p && d_llr, "null argument");
    int per = 0;
    SG_TRY(bpsk_llr_checks(p, B, l0, nl, llr_ld, &per));
    SG_HIP(hipSetDevice(p->device));
    hipStream_t s = pick_stream(stream);
    return by_precision(p->precision, [&](auto t) {
        return bpsk_llr_impl(p, B, l0, nl, llr_ld, probs_only, (decltype(t) *)d_llr, s);
    });
}

int sg_amp_bpsk_llr(sg_amp_plan *p, int B, int l0, int nl, int probs_only, double *out) {
    SG_TRY(ensure_device());
    SG_CHECK_ARG(p && out, "null argument");
    int per = 0;
    SG_TRY(bpsk_llr_checks(p, B, l0, nl, INT32_MAX, &per));
    const int ld = nl * per;  // (<= INT32_MAX: checked)
    return llr_to_host(p, p->device, p->precision, (size_t)B * ld, out, [&](auto *d, hipStream_t s) {
        return bpsk_llr_impl(p, B, l0, nl, ld, probs_only, d, s);
    });
}

// Every refusal of the integrated decoders, before anything is launched or allocated (header, sg_amp_integrated_decode_device)
static int integ_dct_checks(const sg_amp_plan *p, sg_graph *g, int mode, int K, int t_max, int bp_its, int bp_its_final,
                            int *N_out) {
    SG_CHECK_ARG(mode >= SG_INT_NAIVE && mode <= SG_INT_DIFF_POST, "unknown integrated decoder %d", mode);
    if (p->ndim != 0)
        return fail(SG_ERR_UNSUPPORTED, "integrated decoders need a flat design (scalar W), not W.ndim = %d: they "
                    "know one P_l and one tau^2 per codeword", p->ndim);
    if (p->block || p->block2) return fail(SG_ERR_UNSUPPORTED, "no integrated decoder on the block engines");
    if (p->M < 2 || (p->M & (p->M - 1)) != 0 || p->M > 2048)
        return fail(SG_ERR_UNSUPPORTED, "section size M = %d: the integrated section kernel takes a power of two in "
                    "[2, 2048]", p->M);
    int N = 0;
    SG_TRY(sg_ldpc_graph_info(g, &N, nullptr, nullptr, nullptr, nullptr));
    const int logM = ilog2(p->M);
    SG_CHECK_ARG(N > 0 && (p->L * logM) % N == 0, "L log2 M = %d bits must be a multiple of the block length %d",
                 p->L * logM, N);  // ldpc_bp's assert (sparc_new.py:1171)
    SG_CHECK_ARG(K > 0 && K <= N, "bad information length %d", K);
    SG_CHECK_ARG(t_max >= 1 && bp_its >= 0 && bp_its_final >= 0, "bad iteration counts");
    *N_out = N;
    return SG_OK;
}

int sg_amp_integrated_decode_device(sg_amp_plan *p, sg_graph *g, int mode, int K, const void *d_y, int B, int t_max,
                                    int bp_its, int bp_its_final, uint8_t *d_bits, void *d_app, double *d_tau2,
                                    void *stream) {
    SG_CHECK_ARG(p && g && d_y && d_bits, "null argument");
    reset_last(p);  // (the loop runs in the workspace that holds a decode's final state)
    int N = 0;
    SG_TRY(integ_dct_checks(p, g, mode, K, t_max, bp_its, bp_its_final, &N));
    if (B <= 0) return SG_OK;
    SG_TRY(ensure_device());
    SG_HIP(hipSetDevice(p->device));
    hipStream_t s = pick_stream(stream);
    return by_precision(p->precision, [&](auto t) {
        return integ_dct_impl<decltype(t)>(p, g, mode, N, K, d_y, B, t_max, bp_its, bp_its_final, d_bits, d_app,
                                           d_tau2, s);
    });
}

int sg_amp_integrated_decode(sg_amp_plan *p, sg_graph *g, int mode, int K, const double *y, int B, int t_max,
                             int bp_its, int bp_its_final, uint8_t *bits, double *tau2) {
    SG_CHECK_ARG(p && g && y && bits, "null argument");
    reset_last(p);
    int N = 0;
    SG_TRY(integ_dct_checks(p, g, mode, K, t_max, bp_its, bp_its_final, &N));
    if (B <= 0) return SG_OK;
    SG_TRY(ensure_device());
    SG_HIP(hipSetDevice(p->device));
    hipStream_t s = lib_stream();
    const size_t rs = p->precision == SG_F64 ? 8 : 4, ny = (size_t)B * p->n, nt = (size_t)B * t_max;
    const size_t nbits = (size_t)B * (p->L * ilog2(p->M) / N) * K;
    // The workspace before the staging buffer: growing the workspace frees io too (plan_free_ws), so the
    // device entry point's own ensure_ws(p, B, 2) below must find it grown and leave the staging alone
    SG_TRY(ensure_ws(p, B, 2));
    // staging: y as doubles, the tau^2 history, y in the plan precision, the bits
    SG_TRY(ensure_io(p, (ny + nt) * 8 + ny * rs + nbits));
    double *dy = p->io.at<double>(), *dtau = dy + ny;
    void *dyt = dtau + nt;
    uint8_t *dbits = (uint8_t *)dyt + ny * rs;
    SG_HIP(hipMemcpyAsync(dy, y, ny * 8, hipMemcpyHostToDevice, s));
    SG_TRY(by_precision(p->precision, [&](auto t) { return amp_launch_cast(dy, 1, (decltype(t) *)dyt, ny, s); }));
    SG_TRY(sg_amp_integrated_decode_device(p, g, mode, K, dyt, B, t_max, bp_its, bp_its_final, dbits, nullptr,
                                           tau2 ? dtau : nullptr, s));
    SG_HIP(hipMemcpyAsync(bits, dbits, nbits, hipMemcpyDeviceToHost, s));
    if (tau2) SG_HIP(hipMemcpyAsync(tau2, dtau, nt * 8, hipMemcpyDeviceToHost, s));
    SG_HIP(hipStreamSynchronize(s));
    return SG_OK;
}

int sg_amp_count_errors_device(const int32_t *d_map_idx, const int32_t *d_true_idx, const int32_t *d_t_final, int B,
                               int L, int logM, int64_t *d_counts, void *stream) {
    SG_CHECK_ARG(d_map_idx && d_true_idx && d_t_final && d_counts, "null device buffer");
    SG_TRY(ensure_device());
    return amp_launch_count(d_map_idx, d_true_idx, d_t_final, B, L, logM, d_counts, pick_stream(stream));
}

}  // extern "C"
