/* csrc/driver_mix.cpp -- the mixers of the host driver: the wiring (airband_hip_set_mixers / _mixer_enable_input / _mixer_set_stereo / _collect_mixers), what the sums
 * behind a batch's demod kernels are launched with (run_back_half), their exchange between handles over librccl.so (airband_hip_comm_* / *_mixers), and the gated
 * mixer collect over the sums (airband_hip_set_mixer_gate / _mixer_gate_step / _collect_active_mixers / _device_active_mixers / _encode_mixer_audio) with the
 * two readers of its encoded rows: the mixer spool and the mixer RTP stream, whose host sides are driver_gate.cpp's. */
#include <dlfcn.h>

#include "driver.h"

using namespace airband;

MixArgs airband::mix_args(const airband_hip_handle* h) {
    const MixerWiring& w = h->mix;
    MixArgs ma;
    ma.out_wave = h->d_out_wave.p + AB_OUT_PAD;
    ma.wave_stride = h->wave_stride;
    ma.out_axc = h->d_out_axc.p;
    ma.in_chan = w.d_chan.p;
    ma.in_ml = w.d_ml.p;
    ma.in_mr = w.d_mr.p;
    ma.run_first = w.d_run_first.p;
    ma.run_mixer = w.d_run_mixer.p;
    ma.mixer_first_run = w.d_first_run.p;
    ma.mixer_stereo = w.d_stereo.p;
    ma.run_left = w.d_run_left.p;
    ma.run_right = w.d_run_right.p;
    ma.run_signal = w.d_run_signal.p;
    ma.n_runs = w.n_runs;
    ma.left = w.d_left.p;
    ma.right = w.d_right.p;
    ma.has_signal = w.d_signal.p;
    ma.n_mixers = w.n_mixers;
    ma.wave_batch = h->B;
    return ma;
}

/* ---- gated mixer collect (include/airband_hip.h; mixer_gate.hip) ------------------------------------------------------------------- */
static bool mixer_encoding_known(int32_t e) { return e == AIRBAND_AUDIO_F32 || e == AIRBAND_AUDIO_S16 || e == AIRBAND_AUDIO_ULAW || e == AIRBAND_AUDIO_ALAW; }
static size_t mixer_sample_bytes(int e) { return e == AIRBAND_AUDIO_F32 ? 4 : (e == AIRBAND_AUDIO_S16 ? 2 : 1); }
static int mixer_gate_blocks(int n_mixers) { return gate_blocks(n_mixers); } /* the passes are the channel gate's (gate_passes.h) */

/* what the mixer spool and the mixer RTP stream read: the mixer gate's verdicts and the pack's rows and records (airband_hip_set_mixer_spool, _set_mixer_rtp_stream) */
static SpoolSource mixer_spool_source(const airband_hip_handle* h) {
    const MixerGate& g = h->mix_gate;
    SpoolSource src;
    src.mask = g.d_mask.p;
    src.block_count = g.d_block_count.p;
    src.audio = g.d_audio.p;
    src.info = g.d_info.p;
    src.n = h->mix.n_mixers;
    src.max_rows = g.max_rows;
    src.frames = h->B;
    src.width = g.width;
    return src;
}

/* ONE launch path for the automatic step (run_back_half) and the manual one (airband_hip_mixer_gate_step): the list from the sums' signal flags as they are on
 * `s` now, then the listed mixers' rows packed */
void airband::launch_mixer_gate_step(airband_hip_handle* h, hipStream_t s) {
    MixerGate& g = h->mix_gate;
    const MixerWiring& w = h->mix;
    MixerGateArgs a;
    a.gate = g.d_gate.p;
    a.has_signal = w.d_signal.p;
    a.prev = g.d_prev.p;
    a.mask = g.d_mask.p;
    a.block_count = g.d_block_count.p;
    a.index = g.d_index.p;
    a.count = g.d_count.p;
    a.n_mixers = w.n_mixers;
    a.max_rows = g.max_rows;
    launch_mixer_gate_list(a, s);
    MixerPackArgs p;
    p.index = g.d_index.p;
    p.count = g.d_count.p;
    p.n_rows = 0;
    p.max_rows = g.max_rows;
    p.n_mixers = w.n_mixers;
    p.left = w.d_left.p;
    p.right = w.d_right.p;
    p.stereo = w.d_stereo.p;
    p.reserved_all = 0;
    p.out = g.encoding == AIRBAND_AUDIO_F32 ? static_cast<void*>(g.d_rows.p) : static_cast<void*>(g.d_audio.p);
    p.info = g.d_info.p;
    p.wave_batch = h->B;
    p.encoding = g.encoding;
    p.width = g.width;
    launch_mixer_pack(p, 0, s);
    g.stepped = true;
    if (has_mixer_spool(h)) spool_step(g.spool, mixer_spool_source(h), s); /* ... and the mixer spool's step, once per gate step (tx_spool.hip) */
    if (has_mixer_rtp(h)) rtp_step(g.rtp, mixer_spool_source(h), s);       /* ... and the mixer RTP stream's (rtp_stream.hip): another reader of the same rows */
}

/* position k of the grouped mixer-input arrays: the channel it reads, or -1 while the connection (airband_hip_mixer_enable_input) or its dongle
 * (airband_hip_device_enable) is switched off -- a masked input is skipped like mixer->input_mask[i] == false (src/mixer.cpp:96-110,192) */
hipError_t airband::write_mix_input(airband_hip_handle* h, int k) {
    const int ch = h->mix.chan_host[k];
    const int v = (h->mix.user_on[k] && h->dev_enabled[h->plan.cc[ch].dev]) ? ch : -1;
    hipError_t e = hipMemcpyAsync(h->mix.d_chan.p + k, &v, sizeof(int), hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(h->stream); /* `v` is a stack variable */
}

/* ---- the mixer exchange (include/airband_hip.h) ------------------------------------------------------------------------------------ */
namespace {
struct Rccl {
    void* dl = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool named = false;         /* loaded from AIRBAND_HIP_RCCL_LIB */
    bool shared_gpu_ok = false; /* the library says (exported symbol airband_rccl_allows_shared_gpu) that two ranks of a communicator may sit on ONE GPU: the test stand-in does, RCCL does not */
    std::string why;
};
Rccl g_rccl;
std::mutex g_rccl_lock;

/* librccl.so on first use: a process that never exchanges mixer sums never loads it */
Rccl* rccl() {
    std::lock_guard<std::mutex> guard(g_rccl_lock);
    if (g_rccl.dl) return &g_rccl;
    if (!g_rccl.why.empty()) return nullptr;
    void* dl = nullptr;
    std::string tried;
    /* AIRBAND_HIP_RCCL_LIB names the library instead (a site's own RCCL build; the in-process stand-in tests/fake_rccl/ the GPU suite uses to run
     * the exchange with two ranks on a one-GPU box).  Whether two ranks of a communicator may share a GPU is a capability the library exports
     * (airband_rccl_allows_shared_gpu, below): the stand-in has it, RCCL does not. */
    const char* named = getenv("AIRBAND_HIP_RCCL_LIB");
    if (named && *named) {
        dl = dlopen(named, RTLD_NOW | RTLD_GLOBAL);
        if (!dl) {
            const char* e = dlerror(); /* once: dlerror() clears the message it returns */
            tried = std::string(named) + ": " + (e ? e : "not found");
        }
        g_rccl.named = dl != nullptr;
    } else {
        for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
            dl = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (dl) break;
            const char* e = dlerror();
            if (tried.empty()) tried = std::string("librccl.so: ") + (e ? e : "not found");
        }
    }
    if (!dl) {
        g_rccl.why = tried.empty() ? std::string("librccl.so: not found") : tried;
        return nullptr;
    }
#define AB_RCCL_SYM(field, name)                              \
    *(void**)(&g_rccl.field) = dlsym(dl, name);               \
    if (!g_rccl.field) {                                      \
        g_rccl.why = std::string("librccl.so lacks ") + name; \
        dlclose(dl);                                          \
        return nullptr;                                       \
    }
    AB_RCCL_SYM(GetUniqueId, "ncclGetUniqueId") AB_RCCL_SYM(CommInitRank, "ncclCommInitRank") AB_RCCL_SYM(CommInitAll, "ncclCommInitAll")
    AB_RCCL_SYM(AllReduce, "ncclAllReduce") AB_RCCL_SYM(CommDestroy, "ncclCommDestroy") AB_RCCL_SYM(GroupStart, "ncclGroupStart")
    AB_RCCL_SYM(GroupEnd, "ncclGroupEnd") AB_RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef AB_RCCL_SYM
    {   /* a capability the library declares itself, not something inferred from how it was named: a site's own RCCL build named through AIRBAND_HIP_RCCL_LIB
         * keeps the duplicate-GPU check of comm_init_all */
        typedef int (*cap_fn)(void);
        cap_fn cap = reinterpret_cast<cap_fn>(dlsym(dl, "airband_rccl_allows_shared_gpu"));
        g_rccl.shared_gpu_ok = cap && cap() != 0;
    }
    g_rccl.dl = dl;
    return &g_rccl;
}

#define RCCL_TRY(h, R, expr)                                                                                        \
    do {                                                                                                            \
        ncclResult_t r_ = (expr);                                                                                   \
        if (r_ != ncclSuccess) return fail(h, AIRBAND_HIP_ERUNTIME, std::string(#expr ": ") + (R)->GetErrorString(r_)); \
    } while (0)

}  // namespace

extern "C" {

int airband_hip_set_mixers(airband_hip_handle* h, int32_t mixer_count, const airband_hip_mixer_input* in, int32_t n_in) {
    if (!h || mixer_count < 1 || n_in < 0 || (!in && n_in > 0)) return fail(h, AIRBAND_HIP_EINVAL, "bad mixer arguments");
    /* n_in == 0: a handle whose dongles feed no mixer still takes part in the exchange with all-zero partial sums */
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    const Plan& p = h->plan;
    std::vector<int> first(mixer_count + 1, 0), chan(n_in);
    std::vector<float> ml(n_in), mr(n_in);
    std::vector<uint8_t> stereo(mixer_count, 0);
    for (int i = 0; i < n_in; i++) {
        if (in[i].mixer < 0 || in[i].mixer >= mixer_count || in[i].device < 0 || in[i].device >= p.n_dev || in[i].channel < 0 ||
            in[i].channel >= p.dev[in[i].device].n_ch)
            return fail(h, AIRBAND_HIP_EINVAL, "mixer input out of range");
        first[in[i].mixer + 1]++;
        if (in[i].balance != 0.0f) stereo[in[i].mixer] = 1; /* src/mixer.cpp:84-85 */
    }
    for (int m = 0; m < mixer_count; m++) first[m + 1] += first[m];
    std::vector<int> cur(first.begin(), first.end() - 1);
    std::vector<int> pos(n_in, 0);
    for (int i = 0; i < n_in; i++) { /* stable: connection order inside a mixer is kept (summation order) */
        const int k = cur[in[i].mixer]++;
        pos[i] = k;
        chan[k] = p.chan_base[in[i].device] + in[i].channel;
        ml[k] = in[i].ampfactor * fminf(1.0f, 1.0f - in[i].balance); /* src/mixer.cpp:82-83,203-208 */
        mr[k] = in[i].ampfactor * fminf(1.0f, 1.0f + in[i].balance);
    }
    std::vector<int> run_first, run_mixer, first_run(mixer_count + 1, 0);
    for (int m = 0; m < mixer_count; m++) {
        first_run[m] = (int)run_mixer.size();
        for (int i = first[m]; i < first[m + 1]; i += AB_MIX_RUN) {
            run_first.push_back(i);
            run_mixer.push_back(m);
        }
    }
    first_run[mixer_count] = (int)run_mixer.size();
    run_first.push_back(n_in);
    const int n_runs = (int)run_mixer.size();
    /* the mixer kernels index runs / mixers with blockIdx.y: say so here rather than fail at the first launch */
    if (n_runs > 65535 || mixer_count > 65535) return fail(h, AIRBAND_HIP_EBADSIZE, "more than 65 535 mixers (or runs of 64 mixer inputs) on one handle");
    order_behind_last_batch(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream), AIRBAND_HIP_ERUNTIME); /* a batch under way still sums the old wiring */
    h->mix_gate = MixerGate(); /* the gate read the old wiring's sums: it goes with them */
    h->mix = MixerWiring(); /* n_mixers == 0 until the new wiring is complete: a failure below leaves a handle without mixers, not one with freed tables */
    MixerWiring& w = h->mix;
    HIP_TRY(h, upload(w.d_run_first, run_first), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, upload(w.d_run_mixer, run_mixer), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, upload(w.d_first_run, first_run), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, w.d_run_left.alloc((size_t)n_runs * h->B), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, w.d_run_right.alloc((size_t)n_runs * h->B), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, w.d_run_signal.alloc((size_t)n_runs), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, upload(w.d_chan, chan), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, upload(w.d_first, first), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, upload(w.d_ml, ml), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, upload(w.d_mr, mr), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, upload(w.d_stereo, stereo), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, w.d_left.alloc((size_t)mixer_count * h->B), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, w.d_right.alloc((size_t)mixer_count * h->B), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, w.d_signal.alloc((size_t)mixer_count), AIRBAND_HIP_ENOMEM);
    w.pos = pos;
    w.chan_host = chan;
    w.user_on.assign(n_in, 1);
    for (int k = 0; k < n_in; k++) /* inputs of dongles that are already switched off stay out */
        if (!h->dev_enabled[p.cc[chan[k]].dev]) HIP_TRY(h, write_mix_input(h, k), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(h->stream), AIRBAND_HIP_ERUNTIME);
    w.n_runs = n_runs; /* published last */
    w.n_mixers = mixer_count;
    return AIRBAND_HIP_OK;
}

int airband_hip_mixer_enable_input(airband_hip_handle* h, int32_t input_index, int32_t enabled) {
    if (!h || h->mix.n_mixers <= 0) return fail(h, AIRBAND_HIP_EINVAL, "no mixers configured");
    if (input_index < 0 || input_index >= (int32_t)h->mix.pos.size()) return fail(h, AIRBAND_HIP_EINVAL, "mixer input index out of range");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    const int k = h->mix.pos[input_index];
    h->mix.user_on[k] = enabled ? 1 : 0;
    HIP_TRY(h, write_mix_input(h, k), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(h->stream), AIRBAND_HIP_ERUNTIME);
    return AIRBAND_HIP_OK;
}

int airband_hip_mixer_set_stereo(airband_hip_handle* h, int32_t mixer, int32_t stereo) {
    if (!h || h->mix.n_mixers <= 0 || mixer < 0 || mixer >= h->mix.n_mixers) return fail(h, AIRBAND_HIP_EINVAL, "mixer index out of range");
    ON_OWN_STREAM(h, s);
    const uint8_t v = stereo ? 1 : 0;
    HIP_TRY(h, hipMemcpyAsync(h->mix.d_stereo.p + mixer, &v, 1, hipMemcpyHostToDevice, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_mixers(airband_hip_handle* h, float* left, float* right, uint8_t* has_signal) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (h->mix.n_mixers <= 0) return fail(h, AIRBAND_HIP_EINVAL, "no mixers configured");
    ON_OWN_STREAM(h, s);
    const size_t n = (size_t)h->mix.n_mixers * h->B;
    if (left) HIP_TRY(h, hipMemcpyAsync(left, h->mix.d_left.p, n * sizeof(float), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    if (right) HIP_TRY(h, hipMemcpyAsync(right, h->mix.d_right.p, n * sizeof(float), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    if (has_signal) HIP_TRY(h, hipMemcpyAsync(has_signal, h->mix.d_signal.p, (size_t)h->mix.n_mixers, hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    return AIRBAND_HIP_OK;
}

int airband_hip_set_mixer_gate(airband_hip_handle* h, const uint8_t* gate, int64_t max_rows, int32_t encoding, uint32_t flags) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const int n = h->mix.n_mixers;
    if (n <= 0) return fail(h, AIRBAND_HIP_EINVAL, "no mixers configured");
    if (gate) {
        if (max_rows < 1 || max_rows > n) return fail(h, AIRBAND_HIP_EINVAL, "max_rows must lie in 1 .. mixer_count");
        for (int m = 0; m < n; m++)
            if (gate[m] > AIRBAND_GATE_ALWAYS) return fail(h, AIRBAND_HIP_EINVAL, "gate byte of mixer " + std::to_string(m) + " is not an AIRBAND_GATE_* value");
        if (!mixer_encoding_known(encoding)) return fail(h, AIRBAND_HIP_EINVAL, "encoding is not an AIRBAND_AUDIO_* value");
        if (flags & ~(AIRBAND_MIXER_GATE_STEREO | AIRBAND_MIXER_GATE_MANUAL_STEP)) return fail(h, AIRBAND_HIP_EINVAL, "unknown AIRBAND_MIXER_GATE_* flag bits");
        if (h->B % 4) return fail(h, AIRBAND_HIP_EBADSIZE, "the pack kernel moves four frames per lane: WAVE_BATCH must be a multiple of four");
    }
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* built beside the handle and moved in whole: a failed allocation leaves the handle as it was */
    MixerGate g;
    if (gate) {
        const size_t rows = (size_t)max_rows, width = (flags & AIRBAND_MIXER_GATE_STEREO) ? 2 : 1, row_samples = width * (size_t)h->B;
        hipError_t e = upload(g.d_gate, std::vector<uint8_t>(gate, gate + n));
        if (e == hipSuccess) e = g.d_prev.alloc_zeroed((size_t)n);
        if (e == hipSuccess) e = g.d_mask.alloc(((size_t)n + 63) / 64);
        if (e == hipSuccess) e = g.d_block_count.alloc((size_t)mixer_gate_blocks(n));
        if (e == hipSuccess) e = g.d_index.alloc(rows);
        if (e == hipSuccess) e = g.d_count.alloc_zeroed(1);
        if (e == hipSuccess) { /* only what it delivers */
            if (encoding == AIRBAND_AUDIO_F32) e = g.d_rows.alloc(rows * row_samples);
            else e = g.d_audio.alloc(rows * row_samples * mixer_sample_bytes(encoding));
        }
        if (e == hipSuccess && encoding != AIRBAND_AUDIO_F32) e = g.d_info.alloc(rows);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr); /* the zeroes are there before a step on another stream reads them */
        if (e != hipSuccess) return alloc_failed(h, e, "mixer gate buffers: ");
        g.gate.assign(gate, gate + n);
        g.max_rows = (int)max_rows;
        g.encoding = encoding;
        g.width = (int)width;
        g.manual = (flags & AIRBAND_MIXER_GATE_MANUAL_STEP) != 0;
    }
    /* behind the last batch, as airband_hip_set_mixers: a step under way still reads the gate that is replaced here */
    order_behind_last_batch(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream), AIRBAND_HIP_ERUNTIME);
    h->mix_gate = std::move(g);
    return AIRBAND_HIP_OK;
}

int airband_hip_mixer_gate_step(airband_hip_handle* h, void* stream) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_gate(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_GATE);
    if (!h->mix_gate.manual) return fail(h, AIRBAND_HIP_EINVAL, "the mixer gate steps with every batch (set without AIRBAND_MIXER_GATE_MANUAL_STEP)");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* the stream rule of airband_hip_allreduce_mixers: the caller's stream behind the results, or the stream the sums became final on */
    hipStream_t s = stream ? (hipStream_t)stream : results_stream(h);
    if (stream) {
        const int rc = airband_hip_stream_wait_results(h, stream);
        if (rc != AIRBAND_HIP_OK) return rc;
    }
    if (h->ev_last && h->ev_last_pending) HIP_TRY(h, hipStreamWaitEvent(s, h->ev_last, 0), AIRBAND_HIP_ERUNTIME); /* an exchange or a peer's add_mixers on a stream of its own */
    launch_mixer_gate_step(h, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, AIRBAND_HIP_ERUNTIME, std::string("kernel launch: ") + hipGetErrorString(e));
    return results_enqueued_on(h, s); /* collect_active_mixers, and the next batch's sums, come behind the step */
}

int airband_hip_collect_active_mixers(airband_hip_handle* h, int64_t* n_active, int32_t* mixer_index, float* rows, void* audio, airband_hip_audio_row* info, uint8_t* signal_all) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_gate(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_GATE);
    const MixerGate& g = h->mix_gate;
    if (rows && g.encoding != AIRBAND_AUDIO_F32) return fail(h, AIRBAND_HIP_EINVAL, "float rows are delivered by an AIRBAND_AUDIO_F32 mixer gate only");
    if ((audio || info) && g.encoding == AIRBAND_AUDIO_F32) return fail(h, AIRBAND_HIP_EINVAL, "audio and records are delivered by an encoded mixer gate only");
    if (!g.stepped) return AIRBAND_HIP_EAGAIN;
    ON_OWN_STREAM(h, s);
    /* how many rows there are is on the device: the count first, then exactly those entries of each array, ONE synchronize; only then is the count reported */
    int64_t count = 0;
    const int rc = collect_counted<int32_t>(h, g.d_count.p, h->mix.n_mixers, g.max_rows, "active mixer count out of range: ", &count, nullptr, nullptr, s);
    if (rc != AIRBAND_HIP_OK) return rc;
    const size_t n = (size_t)(count < g.max_rows ? count : g.max_rows), row_samples = (size_t)g.width * h->B;
    if (mixer_index && n) HIP_TRY(h, hipMemcpyAsync(mixer_index, g.d_index.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    if (rows && n) HIP_TRY(h, hipMemcpyAsync(rows, g.d_rows.p, n * row_samples * sizeof(float), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    if (audio && n) HIP_TRY(h, hipMemcpyAsync(audio, g.d_audio.p, n * row_samples * mixer_sample_bytes(g.encoding), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    if (info && n) HIP_TRY(h, hipMemcpyAsync(info, g.d_info.p, n * sizeof(airband_hip_audio_row), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    if (signal_all) HIP_TRY(h, hipMemcpyAsync(signal_all, h->mix.d_signal.p, (size_t)h->mix.n_mixers, hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    if (n_active) *n_active = count;
    return AIRBAND_HIP_OK; /* the batch is not marked as collected: airband_hip_collect_mixers() does not do that either */
}

int airband_hip_device_active_mixers(airband_hip_handle* h, int32_t** d_index, int32_t** d_count, float** d_rows, void** d_audio, airband_hip_audio_row** d_info) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_gate(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_GATE);
    const MixerGate& g = h->mix_gate;
    if (d_index) *d_index = g.d_index.p;
    if (d_count) *d_count = g.d_count.p;
    if (d_rows) *d_rows = g.d_rows.p;
    if (d_audio) *d_audio = g.d_audio.p;
    if (d_info) *d_info = g.d_info.p;
    return AIRBAND_HIP_OK;
}

/* ---- mixer transmission spool (include/airband_hip.h; the host side is driver_gate.cpp's, the kernels tx_spool.hip's) ---------------------------------- */
int airband_hip_set_mixer_spool(airband_hip_handle* h, const uint8_t* spool, int64_t pool_rows, int64_t export_rows, int64_t max_records, int32_t min_batches, int32_t idle_batches, int32_t max_batches) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_gate(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_GATE);
    MixerGate& g = h->mix_gate;
    if (g.encoding == AIRBAND_AUDIO_F32) return fail(h, AIRBAND_HIP_EINVAL, "the mixer spool keeps encoded rows: the mixer gate's encoding is AIRBAND_AUDIO_F32");
    if (pool_rows < 0 || export_rows < 0 || max_records < 0 || min_batches < 0 || idle_batches < 0) return fail(h, AIRBAND_HIP_EINVAL, "negative count");
    TransmissionSpool sp; /* built beside the gate and moved in whole: a failed allocation leaves the handle as it was; pool_rows == 0: an empty one, removed */
    if (pool_rows > 0) {
        std::vector<uint8_t> mask;
        int rc = spool_check(h, spool, g.gate, "mixer", pool_rows, export_rows, max_records, max_batches, &mask);
        if (rc != AIRBAND_HIP_OK) return rc;
        HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
        rc = spool_build(h, sp, mask, g.max_rows, (size_t)g.width * h->B * mixer_sample_bytes(g.encoding), pool_rows, export_rows, max_records, min_batches, idle_batches,
                         max_batches, "mixer spool buffers: ");
        if (rc != AIRBAND_HIP_OK) return rc;
    } else {
        HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    }
    /* behind the last batch, as airband_hip_set_mixer_gate: a step under way still reads and writes the spool that is replaced here */
    order_behind_last_batch(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream), AIRBAND_HIP_ERUNTIME);
    g.spool = std::move(sp);
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_mixer_transmissions(airband_hip_handle* h, int64_t* n, airband_hip_transmission* records, void* audio, int64_t* n_rows, int64_t* n_waiting) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_spool(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_SPOOL);
    return spool_collect(h, h->mix_gate.spool, mixer_spool_source(h), n, records, audio, n_rows, n_waiting);
}

int airband_hip_mixer_spool_flush(airband_hip_handle* h) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_spool(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_SPOOL);
    return spool_flush(h, h->mix_gate.spool, mixer_spool_source(h));
}

int airband_hip_mixer_spool_counters_get(airband_hip_handle* h, airband_hip_spool_counters* out) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_spool(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_SPOOL);
    return spool_counters(h, h->mix_gate.spool, out);
}

int airband_hip_device_mixer_spool(airband_hip_handle* h, void** d_export_audio, airband_hip_transmission** d_export_records, int32_t** d_n_export) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_spool(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_SPOOL);
    spool_device_views(h->mix_gate.spool, d_export_audio, d_export_records, d_n_export);
    return AIRBAND_HIP_OK;
}

/* ---- mixer RTP stream (include/airband_hip.h; the host side is driver_gate.cpp's, the kernels rtp_stream.hip's) ------------------------------------------- */
int airband_hip_mixer_rtp_slot_bytes(int32_t encoding, int32_t frame_samples, int32_t width) { return rtp_slot_bytes_checked(encoding, frame_samples, width); }

int airband_hip_set_mixer_rtp_stream(airband_hip_handle* h, const airband_hip_rtp_source* sources, int32_t frame_samples, int64_t max_packets) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_gate(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_GATE);
    MixerGate& g = h->mix_gate;
    if (g.encoding == AIRBAND_AUDIO_F32) return fail(h, AIRBAND_HIP_EINVAL, "the mixer RTP stream frames encoded rows: the mixer gate's encoding is AIRBAND_AUDIO_F32");
    RtpStream r; /* built beside the gate and moved in whole: a failed allocation leaves the handle as it was; sources == NULL: an empty one, removed */
    if (sources) {
        const int rc = rtp_build(h, r, sources, g.gate, "mixer", g.encoding, mixer_spool_source(h), frame_samples, max_packets, "mixer RTP stream buffers: ");
        if (rc != AIRBAND_HIP_OK) return rc;
    } else {
        HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    }
    /* behind the last batch, as airband_hip_set_mixer_spool: a step under way still reads and writes the stream that is replaced here */
    order_behind_last_batch(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream), AIRBAND_HIP_ERUNTIME);
    g.rtp = std::move(r);
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_mixer_rtp_packets(airband_hip_handle* h, int64_t* n_packets, airband_hip_rtp_packet* records, void* packets, uint8_t* signal_all) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_rtp(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_RTP);
    if (!h->mix_gate.rtp.has_result) return AIRBAND_HIP_EAGAIN;
    /* the batch is not marked as collected: airband_hip_collect_active_mixers() does not do that either */
    return rtp_collect(h, h->mix_gate.rtp, mixer_spool_source(h), n_packets, records, packets, h->mix.d_signal.p, signal_all, (size_t)h->mix.n_mixers);
}

int airband_hip_collect_mixer_rtp_state(airband_hip_handle* h, int64_t first_mixer, int64_t n_mixers, airband_hip_rtp_state* state) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_rtp(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_RTP);
    return rtp_state(h, h->mix_gate.rtp, mixer_spool_source(h), first_mixer, n_mixers, state, "mixer");
}

int airband_hip_mixer_rtp_counters_get(airband_hip_handle* h, airband_hip_rtp_counters* out) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_rtp(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_RTP);
    return rtp_counters(h, h->mix_gate.rtp, out);
}

int airband_hip_mixer_rtp_flush(airband_hip_handle* h) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_rtp(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_RTP);
    return rtp_flush(h, h->mix_gate.rtp, mixer_spool_source(h));
}

int airband_hip_device_mixer_rtp_stream(airband_hip_handle* h, int32_t** d_n_packets, airband_hip_rtp_packet** d_records, void** d_packets, airband_hip_rtp_state** d_state) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_mixer_rtp(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_MIXER_RTP);
    rtp_device_views(h->mix_gate.rtp, d_n_packets, d_records, d_packets, d_state);
    return AIRBAND_HIP_OK;
}

int airband_hip_encode_mixer_audio(airband_hip_handle* h, int32_t encoding, const float* left, const float* right, int64_t n_rows, void* audio, airband_hip_audio_row* info) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!left) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    if (encoding == AIRBAND_AUDIO_F32 || !mixer_encoding_known(encoding)) return fail(h, AIRBAND_HIP_EINVAL, "encoding is not AIRBAND_AUDIO_S16, _ULAW or _ALAW");
    if (n_rows < 0 || n_rows > 0x7fffffff / 8) return fail(h, AIRBAND_HIP_EINVAL, "n_rows out of range");
    if (h->B % 4) return fail(h, AIRBAND_HIP_EBADSIZE, "the pack kernel moves four frames per lane: WAVE_BATCH must be a multiple of four");
    if (n_rows == 0) return AIRBAND_HIP_OK;
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* buffers of the call's own, on the null stream: nothing of the handle is read or written */
    const size_t n = (size_t)n_rows, B = (size_t)h->B, width = right ? 2 : 1, row_bytes = width * B * mixer_sample_bytes(encoding);
    DevBuf<float> d_left, d_right;
    DevBuf<uint8_t> d_audio;
    DevBuf<airband_hip_audio_row> d_info;
    hipError_t e = d_left.alloc(n * B);
    if (e == hipSuccess && right) e = d_right.alloc(n * B);
    if (e == hipSuccess) e = d_audio.alloc(n * row_bytes);
    if (e == hipSuccess) e = d_info.alloc(n);
    if (e != hipSuccess) return alloc_failed(h, e, "encode_mixer_audio buffers: ");
    HIP_TRY(h, hipMemcpy(d_left.p, left, n * B * sizeof(float), hipMemcpyHostToDevice), AIRBAND_HIP_ERUNTIME);
    if (right) HIP_TRY(h, hipMemcpy(d_right.p, right, n * B * sizeof(float), hipMemcpyHostToDevice), AIRBAND_HIP_ERUNTIME);
    MixerPackArgs a;
    a.index = nullptr;
    a.count = nullptr;
    a.n_rows = (int)n_rows;
    a.max_rows = (int)n_rows;
    a.n_mixers = (int)n_rows;
    a.left = d_left.p;
    a.right = d_right.p;
    a.stereo = nullptr;
    a.reserved_all = right ? 1u : 0u;
    a.out = d_audio.p;
    a.info = d_info.p;
    a.wave_batch = h->B;
    a.encoding = encoding;
    a.width = (int)width;
    launch_mixer_pack(a, 0, nullptr);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(h, AIRBAND_HIP_ERUNTIME, std::string("kernel launch: ") + hipGetErrorString(e));
    if (audio) HIP_TRY(h, hipMemcpy(audio, d_audio.p, n * row_bytes, hipMemcpyDeviceToHost), AIRBAND_HIP_ERUNTIME);
    if (info) HIP_TRY(h, hipMemcpy(info, d_info.p, n * sizeof(airband_hip_audio_row), hipMemcpyDeviceToHost), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(nullptr), AIRBAND_HIP_ERUNTIME); /* the buffers go with this call */
    return AIRBAND_HIP_OK;
}

int airband_hip_comm_unique_id(uint8_t id[AIRBAND_HIP_COMM_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == AIRBAND_HIP_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    Rccl* R = rccl();
    if (!R) return fail(nullptr, AIRBAND_HIP_ENODEV, g_rccl.why);
    ncclUniqueId u;
    RCCL_TRY(nullptr, R, R->GetUniqueId(&u));
    memcpy(id, &u, sizeof(u));
    return AIRBAND_HIP_OK;
}

int airband_hip_comm_init_rank(airband_hip_handle* h, const uint8_t id[AIRBAND_HIP_COMM_ID_BYTES], int32_t nranks, int32_t rank) {
    if (!h || !id || nranks < 1 || rank < 0 || rank >= nranks) return fail(h, AIRBAND_HIP_EINVAL, "bad communicator arguments");
    if (h->comm) return fail(h, AIRBAND_HIP_EINVAL, "the handle already has a communicator");
    Rccl* R = rccl();
    if (!R) return fail(h, AIRBAND_HIP_ENODEV, g_rccl.why);
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    RCCL_TRY(h, R, R->CommInitRank(&h->comm, nranks, u, rank));
    return AIRBAND_HIP_OK;
}

int airband_hip_comm_init_all(airband_hip_handle** hs, int32_t n) {
    if (!hs || n < 1) return fail(nullptr, AIRBAND_HIP_EINVAL, "bad communicator arguments");
    std::vector<int> devs(n);
    for (int i = 0; i < n; i++) {
        if (!hs[i] || hs[i]->comm) return fail(hs[i], AIRBAND_HIP_EINVAL, "NULL handle, or a handle that already has a communicator");
        devs[i] = hs[i]->hip_device;
        if (hs[i]->mix.n_mixers != hs[0]->mix.n_mixers || hs[i]->B != hs[0]->B) return fail(hs[i], AIRBAND_HIP_EINVAL, "the handles of a clique need the same mixer_count and WAVE_BATCH");
    }
    Rccl* R = rccl();
    if (!R) return fail(hs[0], AIRBAND_HIP_ENODEV, g_rccl.why);
    if (!R->shared_gpu_ok) /* RCCL proper refuses a communicator with one GPU twice, late and with a generic message */
        for (int i = 0; i < n; i++)
            for (int k = 0; k < i; k++)
                if (devs[k] == devs[i]) return fail(hs[i], AIRBAND_HIP_EINVAL, "two handles of the clique share a GPU: use airband_hip_add_mixers between them");
    std::vector<ncclComm_t> comms(n, nullptr);
    RCCL_TRY(hs[0], R, R->CommInitAll(comms.data(), n, devs.data()));
    for (int i = 0; i < n; i++) hs[i]->comm = comms[i];
    return AIRBAND_HIP_OK;
}

int airband_hip_comm_group_begin(void) {
    Rccl* R = rccl();
    if (!R) return fail(nullptr, AIRBAND_HIP_ENODEV, g_rccl.why);
    RCCL_TRY(nullptr, R, R->GroupStart());
    return AIRBAND_HIP_OK;
}

int airband_hip_comm_group_end(void) {
    Rccl* R = rccl();
    if (!R) return fail(nullptr, AIRBAND_HIP_ENODEV, g_rccl.why);
    RCCL_TRY(nullptr, R, R->GroupEnd());
    return AIRBAND_HIP_OK;
}

/* SUM of the mixer waveforms (src/mixer.cpp:133-140), MAX of the signal flags (channel->axcindicate = SIGNAL if any input had signal, :209), in place */
int airband_hip_allreduce_mixers(airband_hip_handle* h, void* stream) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (h->mix.n_mixers <= 0) return fail(h, AIRBAND_HIP_EINVAL, "no mixers configured");
    if (!h->comm) return fail(h, AIRBAND_HIP_EINVAL, "no communicator: airband_hip_comm_init_rank / _init_all first");
    Rccl* R = rccl();
    if (!R) return fail(h, AIRBAND_HIP_ENODEV, g_rccl.why);
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    hipStream_t s = stream ? (hipStream_t)stream : results_stream(h);
    if (stream) {
        const int rc = airband_hip_stream_wait_results(h, stream);
        if (rc != AIRBAND_HIP_OK) return rc;
    }
    const size_t n = (size_t)h->mix.n_mixers * h->B;
    RCCL_TRY(h, R, R->GroupStart());
    RCCL_TRY(h, R, R->AllReduce(h->mix.d_left.p, h->mix.d_left.p, n, ncclFloat, ncclSum, h->comm, s));
    RCCL_TRY(h, R, R->AllReduce(h->mix.d_right.p, h->mix.d_right.p, n, ncclFloat, ncclSum, h->comm, s));
    RCCL_TRY(h, R, R->AllReduce(h->mix.d_signal.p, h->mix.d_signal.p, (size_t)h->mix.n_mixers, ncclUint8, ncclMax, h->comm, s));
    RCCL_TRY(h, R, R->GroupEnd());
    return results_enqueued_on(h, s); /* whatever the handle does next to these buffers (the next batch's sums, collect_mixers) comes behind the exchange */
}

int airband_hip_add_mixers(airband_hip_handle* dst, airband_hip_handle* src) {
    if (!dst || !src || dst == src) return fail(dst, AIRBAND_HIP_EINVAL, "two different handles needed");
    if (dst->mix.n_mixers <= 0 || dst->mix.n_mixers != src->mix.n_mixers || dst->B != src->B) return fail(dst, AIRBAND_HIP_EINVAL, "the handles need the same mixer_count and WAVE_BATCH");
    if (dst->hip_device != src->hip_device) return fail(dst, AIRBAND_HIP_EINVAL, "handles on different GPUs exchange through airband_hip_allreduce_mixers");
    HIP_TRY(dst, hipSetDevice(dst->hip_device), AIRBAND_HIP_ENODEV);
    HIP_TRY(dst, dst->ev_peer.ensure(), AIRBAND_HIP_ENODEV);
    hipStream_t s = results_stream(dst);
    HIP_TRY(dst, hipEventRecord(dst->ev_peer, results_stream(src)), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(dst, hipStreamWaitEvent(s, dst->ev_peer, 0), AIRBAND_HIP_ERUNTIME);
    launch_mix_add(dst->mix.d_left.p, dst->mix.d_right.p, dst->mix.d_signal.p, src->mix.d_left.p, src->mix.d_right.p, src->mix.d_signal.p, dst->mix.n_mixers, dst->B, s);
    /* src's next batch must not overwrite its sums before they have been read */
    const int rc_mark = results_enqueued_on(src, s);
    if (rc_mark != AIRBAND_HIP_OK) return rc_mark;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(dst, AIRBAND_HIP_ERUNTIME, std::string("mixer add launch: ") + hipGetErrorString(e));
    return AIRBAND_HIP_OK;
}

/* A handle that ran no batch this round (every dongle of it switched off) still stands in the exchange: its partial sums are those of a
 * mixer whose inputs are all masked out (mixer_disable_input(), src/mixer.cpp:96-112) -- zeros, no signal.  Its buffers do NOT hold that by
 * themselves: the last batch's sums are still in them, and after an in-place all-reduce the whole node's. */
int airband_hip_clear_mixers(airband_hip_handle* h) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (h->mix.n_mixers <= 0) return fail(h, AIRBAND_HIP_EINVAL, "no mixers configured");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    hipStream_t s = results_stream(h); /* behind whatever wrote or read the sums last: the handle's last batch, an exchange, add_mixers */
    if (h->ev_last && h->ev_last_pending) HIP_TRY(h, hipStreamWaitEvent(s, h->ev_last, 0), AIRBAND_HIP_ERUNTIME); /* a peer's add_mixers still reading them */
    const size_t n = (size_t)h->mix.n_mixers * h->B;
    HIP_TRY(h, hipMemsetAsync(h->mix.d_left.p, 0, n * sizeof(float), s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipMemsetAsync(h->mix.d_right.p, 0, n * sizeof(float), s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipMemsetAsync(h->mix.d_signal.p, 0, (size_t)h->mix.n_mixers, s), AIRBAND_HIP_ERUNTIME);
    return results_enqueued_on(h, s); /* collect_mixers, or a later batch on another stream, comes behind the clear -- as behind allreduce_mixers */
}

int airband_hip_comm_destroy(airband_hip_handle* h) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!h->comm) return AIRBAND_HIP_OK;
    Rccl* R = rccl();
    if (R) {
        (void)hipSetDevice(h->hip_device);
        (void)hipStreamSynchronize(h->stream);
        (void)R->CommDestroy(h->comm);
    }
    h->comm = nullptr;
    return AIRBAND_HIP_OK;
}

} /* extern "C" */
