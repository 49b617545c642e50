/*
 * audioforge_mi.h -- C ABI of the MI355X-native batched voice-DSP engine.
 *
 * The reference (FueledByRedBull/audio-forge, rust-core) exposes its per-frame voice
 * chain to Python through PyO3 (`mic_eq.mic_eq_core`, rust-core/src/lib.rs:301-350);
 * it has no C ABI of its own.  This header is the boundary a maintainer binds instead
 * (ctypes / cffi / pyo3-ffi): an `af_engine` is N independent copies of the reference's
 * `OfflineDspBlockProcessor` (rust-core/src/audio/processor/block_processor.rs:31-60),
 * one per 48 kHz mono stream, resident on one GPU, driven through the same setter
 * surface the reference's structs have.  Every entry point cites the reference method
 * it replaces.  All functions return 0 (AF_OK) or a negative af_status; the message of
 * the last failure on the calling thread is af_last_error().
 *
 * Threading: an engine is not thread safe; use one host thread per engine/device.
 * Ownership: every buffer is caller-owned; the engine copies what it keeps.
 */
#ifndef AUDIOFORGE_MI_H
#define AUDIOFORGE_MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum af_status {
  AF_OK = 0,
  AF_ERR_INVALID_ARGUMENT = -1, /* PyValueError in the reference binding            */
  AF_ERR_BACKEND = -2,          /* PyRuntimeError: HIP failure / no device          */
  AF_ERR_NON_FINITE = -3,       /* "audio must contain only finite samples"         */
  AF_ERR_STATE = -4,            /* configuration setter used after streaming started, or
                                   any chain setter then with live control off (below) */
  AF_ERR_UNSUPPORTED = -5
} af_status;

typedef struct af_engine af_engine;

/* ---- stable public filter ids: rust-core/src/dsp/eq.rs:44-53 ---- */
enum { AF_EQ_LOW_SHELF = 0, AF_EQ_BELL = 1, AF_EQ_HIGH_SHELF = 2, AF_EQ_NOTCH = 3,
       AF_EQ_HIGH_PASS = 4, AF_EQ_LOW_PASS = 5 };

/* EqBandConfig, rust-core/src/dsp/eq.rs:112-120 */
typedef struct af_eq_band_config {
  int32_t filter_type;
  double frequency_hz;
  double gain_db;
  double q;
  int32_t slope_db_per_octave;
  int32_t enabled;
} af_eq_band_config;

/* OfflineDspBlockStats (block_processor.rs:1-28) + the two per-block energy sums that
 * simulate_auto_eq_chain accumulates around each block (python_api.rs:515-553). */
typedef struct af_block_stats {
  float input_sample_peak;
  float output_sample_peak;
  float true_peak_limiter_input_peak;
  float output_true_peak;
  float limiter_peak_gain_reduction_db;
  float true_peak_limiter_gain_reduction_db;
  float compressor_gain_reduction_db;
  float deesser_gain_reduction_db;
  double input_square_sum;
  double output_square_sum;
  uint32_t true_peak_limited_events; /* 0 or 1 per block, true_peak.rs:376 */
  uint32_t non_finite_output;
  /* Compressor::current_makeup_gain / auto_makeup_activity / auto_makeup_activity_reliability at the end of
   * the block (compressor.rs:346-363) -- the traces of simulate_auto_makeup_control */
  float compressor_makeup_gain_db;
  float auto_makeup_activity;
  float auto_makeup_reliability;
  float reserved;
} af_block_stats;

/* layout of the audio buffers handed to af_engine_process_* */
enum { AF_LAYOUT_STREAM_MAJOR = 0 /* [stream][time] */, AF_LAYOUT_TIME_MAJOR = 1 /* [time][stream] */ };

/* kernel variants (all produce the same samples) */
enum { AF_KERNEL_AUTO = 0, AF_KERNEL_LANE_PER_STREAM = 1, AF_KERNEL_PHASED = 2, AF_KERNEL_QUAD = 3, AF_KERNEL_STAGED = 4,
       AF_KERNEL_ROLES = 5 /* wave roles inside one workgroup per 64 streams, LDS hand-over (csrc/af_roles.hip) */ };

int af_version(void);
const char *af_last_error(void);
/* number of HIP devices visible; negative status when the runtime is unusable */
int af_device_count(void);

/* ---- lifecycle ------------------------------------------------------------------ */
/* OfflineDspBlockProcessor::new(sample_rate), block_processor.rs:46-60, for
 * `n_streams` independent streams on HIP device `device`.  No GPU work happens until
 * the first af_engine_process_* call (configuration is pure host work). */
int af_engine_create(double sample_rate, int32_t n_streams, int32_t device, af_engine **out);
void af_engine_destroy(af_engine *engine);
/* Re-arm every stream with the configured initial state (a fresh processor with the
 * same setter history); afterwards setters are accepted again. */
int af_engine_reset(af_engine *engine);
int32_t af_engine_n_streams(const af_engine *engine);

/* Setters mirror the reference structs.  Until the first af_engine_process_* / af_engine_stream_* call every setter is
 * accepted (configuration mode); af_engine_reset returns the engine to that mode.
 *
 * After streaming started a CONFIGURATION setter returns AF_ERR_STATE: the stage enables and af_engine_set_eq_before_deesser
 * (they change which kernels and stages are resident), af_limiter_set_lookahead_ms (ring and LDS sizes),
 * af_compressor_set_auto_makeup_enabled (the kernel form and the state planes' size are chosen per value), af_eq_reset,
 * af_engine_set_control_block_samples, the scrub / clamp / pre-filter switches, preset count and assignment, kernel selection,
 * af_engine_set_live_control, and every setter documented below as a configuration setter.
 *
 * The other chain setters (af_eq_set_band_*, af_compressor_set_*, af_limiter_set_ceiling / _release_time,
 * af_true_peak_limiter_set_release_ms, af_deesser_set_*) are LIVE setters.  With live control off (the default) they too
 * return AF_ERR_STATE after streaming started.  With af_engine_set_live_control(e, 1) they are accepted between calls and
 * act like the reference's realtime control plane (audio/processor/control.rs:844-919 applied at the top of a wake-up,
 * dsp_loop.rs:604-637): the reference setter's effect on the RUNNING object -- a coefficient crossfade that starts from the
 * live filter memories (biquad.rs:249-260), the compressor's release fields and release envelopes (compressor.rs:210-275),
 * the side-chain reset on a toggle (compressor.rs:366-371) -- lands at the first sample the chain processes in the next
 * call, for every stream of the selected preset, in the order the setters were called.  Per-stream state is edited on the
 * device by one extra kernel launch in front of that call; a call with nothing pending launches nothing extra.
 * Arguments are checked first: a live EQ setter validates the band it would produce with EqBandConfig::validate
 * (af_eq_band_config_validate: AF_ERR_INVALID_ARGUMENT and the same message), and a refused setter leaves nothing pending.
 * Refused live with AF_ERR_UNSUPPORTED, nothing pending: an EQ band change that needs more biquad sections than the band
 * holds (the state planes are sized at start);
 * af_compressor_set_adaptive_release / _sidechain_highpass_enabled on a multi-preset engine that runs the stage pipeline
 * (its presets must take the same code paths).
 * af_engine_reset keeps the switch, drops what is pending, and re-arms a preset that was retuned live like the reference's
 * reset(): every filter starts from its configured target (Biquad::reset, biquad.rs:341-347).
 * Setters and process calls of one engine are single-threaded, as everywhere in this header. */
int af_engine_set_live_control(af_engine *e, int32_t enabled);  /* a configuration setter; off by default */
/* state edits recorded since the last call that ran the chain (0 with nothing pending); `ops` may be null */
int af_engine_live_control_pending(const af_engine *e, int32_t *ops);
/* with af_engine_set_timing_enabled: device time of the last call's state-retune launch, 0 when it launched none (synchronises) */
int af_engine_last_retune_ms(af_engine *e, double *ms);

/* ---- per-stream lifecycle: restart, export and import single streams of a running engine ----------------------------
 * In the reference every stream is its own AudioProcessor with its own reset() and lifetime.  With
 * af_engine_set_stream_lifecycle(e, 1) (a configuration setter, off by default: with it off every call, kernel choice and
 * bit is as without it) a started engine accepts the calls below BETWEEN process calls.  With the switch on AF_KERNEL_AUTO
 * never selects the stage pipeline (its hand-over rings hold the histories) and takes the forms it takes above the
 * pipeline's stream limit; an engine forced to AF_KERNEL_STAGED is refused at its first process call (AF_ERR_UNSUPPORTED).
 *
 * `streams` is a host array of n DISTINCT stream indices (a duplicate or an index out of range: AF_ERR_INVALID_ARGUMENT);
 * n = 0 does nothing.  Every call is one kernel launch on the stream of the last process call; restart and import do not
 * wait for the device, export waits for its one copy to the host.  Every stream not listed is untouched.
 *
 * af_engine_restart_streams: the listed streams continue from the state a fresh engine gives them -- their preset's
 *   initial chain state, the suppressor's initial row, a zero gate row (Biquad::reset to the configured target,
 *   NoiseGate::reset, rnnoise.rs:205-210) -- and their own sample count restarts at 0.  (The reference's reset(): where
 *   configuration setters scheduled a coefficient crossfade -- EQ bands, de-esser cuts -- a fresh engine plays it in its
 *   first samples; its counters belong to the preset, so a restarted stream starts at the configured target instead.)
 * af_engine_export_stream_state: n blobs of af_engine_stream_state_size bytes each, back to back.  A blob is CANONICAL: it
 *   does not depend on the engine's absolute sample count (the limiter's delay ring is stored oldest input first, its
 *   block maxima are not stored), so the same stream history gives the same bytes in any engine.  It starts with a header
 *   (magic, version, sizes, sample rate, control block, the shape of the slot's preset and of the engine's state planes,
 *   the stream's own sample count); layout: DESIGN.md 4.24 and csrc/af_stream_state.h.
 * af_engine_import_stream_state: each blob's header is checked against its destination slot first: a wrong magic or
 *   version or a shape that differs gives AF_ERR_INVALID_ARGUMENT, the message names the field, and nothing is touched.
 *   Parameter VALUES may differ between source and destination; that is the caller's business, as with live control.  The
 *   ring is placed at this engine's phase and the maxima are recomputed, so the stream continues bit for bit.
 * af_engine_stream_samples_processed: samples the stream has run since its own (re)start, an import carrying the count over.
 *
 * Refused with AF_ERR_UNSUPPORTED, nothing touched, the message naming the rule: samples pending in the suppressor's frame
 * assembly (af_engine_pending_input), an engine sample count that is not a whole number of control blocks, a coefficient
 * crossfade in flight in any preset, live-control edits pending, the stage pipeline active or selected, the VAD-fused gate
 * attached, and device-rate I/O, multichannel input or the output writer set (they keep per-stream state of their own).
 * AF_ERR_STATE: the switch is off, or streaming has not started.  All of these are decided before any device call. */
int af_engine_set_stream_lifecycle(af_engine *e, int32_t enabled);
int af_engine_restart_streams(af_engine *e, const int32_t *streams, int32_t n);
int af_engine_stream_state_size(af_engine *e, size_t *bytes);  /* one blob of this engine; valid in configuration mode too */
int af_engine_export_stream_state(af_engine *e, const int32_t *streams, int32_t n, void *blobs /* [n][bytes] host */);
int af_engine_import_stream_state(af_engine *e, const int32_t *streams, int32_t n, const void *blobs);
int af_engine_stream_samples_processed(const af_engine *e, int32_t stream, int64_t *samples);

/* ---- chain switches: block_processor.rs:62-84 ----------------------------------- */
int af_engine_set_deesser_enabled(af_engine *e, int32_t enabled);
int af_engine_set_eq_enabled(af_engine *e, int32_t enabled);
int af_engine_set_compressor_enabled(af_engine *e, int32_t enabled);
int af_engine_set_limiter_enabled(af_engine *e, int32_t enabled);
int af_engine_set_eq_before_deesser(af_engine *e, int32_t enabled);
/* Samples per reference block: python_api.rs:512-514 uses round(0.020*fs)=960,
 * the golden test 480 (tests.rs:1825).  Each af_engine_process_* call is cut into
 * blocks of this size (last one short), exactly like `audio.chunks(n)`. */
int af_engine_set_control_block_samples(af_engine *e, int32_t samples);
/* python_api.rs:517-520: non-finite input samples become 0 (on by default) */
int af_engine_set_input_scrub_enabled(af_engine *e, int32_t enabled);

/* ---- realtime front end (off by default: the offline simulator has none) -------- */
/* sanitize_and_clamp_input_inplace, audio/processor/routing.rs:802-823 */
int af_engine_set_input_clamp_enabled(af_engine *e, int32_t enabled);
/* apply_input_pre_filter: DC block + 80 Hz high-pass, routing.rs:826-843 */
int af_engine_set_prefilter_enabled(af_engine *e, int32_t enabled, int32_t apply_fixed_highpass);

/* ---- noise gate stage: rust-core/src/dsp/gate.rs (NoiseGate) as stage 1 of the realtime loop -------------------
 * Realtime order (dsp_loop.rs:1371-1435, built at :478-487 as NoiseGate::new(-40, 10, 100, fs)): input scrub / clamp ->
 * DC block + 80 Hz high-pass -> GATE -> suppressor (whose dry signal is the gated one) -> de-esser / EQ / compressor /
 * limiter / true peak.  Per stream, process_block_inplace on the path without a VadAutoGate: update_detector
 * (gate.rs:265-285), detector_gain_reduction_db with the auto-relax range (:298-306), track_gate_transition (:578-611),
 * apply_gain (:613-623), process_sample (:626-637).  Modes 1 (VadAssisted) and 2 (VadOnly) arm the chatter auto-relax
 * (24 dB floor) as that path does; the realtime loop also attaches VadAutoGate::without_backend, whose fused-probability
 * path runs once the controller is attached (af_gate_set_vad_auto_gate_enabled, below).
 * Off by default.  Parameters are engine-wide (presets do not carry them) and live between process calls, like
 * apply_gate_control (processor/control.rs:851-865): threshold [-80, -10] dB, attack [0.1, 100] ms, release [10, 1000] ms
 * (audio/processor.rs:77-82); a non-finite value leaves the setting unchanged (control.rs:50-52).  Mode 0/1/2, anything
 * else is AF_ERR_INVALID_ARGUMENT "Invalid gate mode" (gate_controls.rs:75-81); mode 0 clears the auto-relax counter
 * (gate.rs:812-821).  State is per stream: disabling freezes it, re-enabling resumes from it, af_engine_reset restores
 * NoiseGate::reset (gate.rs:759-785).  Stream-major audio only (AF_ERR_UNSUPPORTED otherwise; also for a gate-off call of an
 * engine whose stage-pipeline route was chosen with the gate on and the front end in the gate's pre-pass).  With the suppressor off
 * the chain receives the gated front-end output, and the block input statistics describe that signal. */
int af_engine_set_gate_enabled(af_engine *e, int32_t enabled);
int af_gate_set_threshold(af_engine *e, double threshold_db);
int af_gate_set_attack_time(af_engine *e, double attack_ms);
int af_gate_set_release_time(af_engine *e, double release_ms);
int af_gate_set_mode(af_engine *e, int32_t mode);
double af_gate_threshold_db(const af_engine *e);      /* VALUE */
int32_t af_engine_gate_enabled(const af_engine *e);   /* VALUE */
/* each stream's gate as of the end of the last call (synchronises): current_gain = NoiseGate::current_gain, chatter
 * events since reset, flags bit 0 is_open, bit 1 auto_relax_active -- what dsp_loop.rs:1397-1409 publishes to the
 * meters.  Any pointer may be null; n_streams <= the engine's. */
int af_engine_read_gate_state(af_engine *e, float *current_gain, uint64_t *chatter_events, int32_t *flags, int32_t n_streams);
/* ---- the VAD-fused gate modes: the gate with a VadAutoGate::without_backend attached, as the realtime loop runs it -------
 * dsp_loop.rs:478-487 attaches VadAutoGate::without_backend(fs, vad_threshold) to stage 1 and hands the gate one speech
 * probability per block (set_external_vad_probability, dsp_loop.rs:1381-1397).  With the controller attached and mode 1 or 2
 * the gate takes the branch at gate.rs:657-741: per control block the controller (vad.rs:714-966: block RMS in f32, noise-floor
 * histogram with auto-threshold, debounce and hold time), per sample the fused score (gate.rs:315-366), the five-state
 * probabilistic gate (:374-483) and the continuous posterior reduction (:485-553).  The probability comes from the caller: no
 * Silero, no model.  Detached (the default) every mode behaves as described above; attached and mode 0 is the expander, and the
 * controller is not stepped (gate.rs:659, 743-745).
 * af_gate_set_vad_auto_gate_enabled: NoiseGate::set_vad_auto_gate (gate.rs:829-836).  A newly attached controller starts from
 *   without_backend's state (vad.rs:663-690); its manual threshold IS the gate's threshold (af_gate_set_threshold feeds both,
 *   gate.rs:227-233).  The controller's SETTINGS below are engine-wide and kept while detached (the reference's setters are
 *   no-ops without a controller and a new controller starts from its defaults: set them again after attaching to get that).
 * af_gate_set_vad_threshold [0, 1] (vad.rs:1043; default 0.48, control.rs:89), af_gate_set_hold_time [0, 500] ms (vad.rs:1054;
 *   200), af_gate_set_margin [0, 20] dB (vad.rs:984; 10), af_gate_set_auto_threshold (vad.rs:1002; on): live between calls like
 *   apply_gate_control (control.rs:856-864); a non-finite value leaves the setting as it is.  set_vad_pre_gain is LEFT OUT: it
 *   only reaches a Silero instance (vad.rs:1069-1073), which this engine does not have.
 * af_gate_set_vad_evidence: for the NEXT process call whose gate pass runs the fused path, one probability (clamped to [0, 1],
 *   gate.rs:841) and one availability flag per control block of the samples that pass covers (the call, or behind the suppressor
 *   the whole frames it completes; last block short: the cut of the block statistics), shared by all streams or
 *   [block][stream].  Consumed by that call.  n_blocks = 0 clears it; without evidence every block runs with probability 0, not
 *   available (dsp_loop.rs:1387-1395 with a stale worker).  Detaching the controller or selecting mode 0 drops it.  A call whose block count differs is refused with
 *   AF_ERR_INVALID_ARGUMENT before anything is touched.
 * af_engine_read_gate_vad_state (synchronises): what dsp_loop.rs:1410-1431 publishes -- noise_floor(), noise_floor_reliability(),
 *   fused_gate_score(), get_vad_probability() (the smoothed posterior) -- plus gate_state (0 Closed, 1 Opening, 2 Open,
 *   3 Uncertain, 4 Releasing) and flags: bit 0 the last block's held-open decision, bit 1 fused_gate_open, bit 2 the last
 *   block's availability.  Null pointers are skipped.  Detached: -60, 0 (gate.rs:935-951).
 * af_engine_reset restores NoiseGate::reset + VadAutoGate::reset (the closed counter restarts at 50 ms, vad.rs:1022) and drops
 * pending evidence; af_gate_set_mode(0) also puts gate_state back to Closed (gate.rs:814-817). */
int af_gate_set_vad_auto_gate_enabled(af_engine *e, int32_t enabled);
int af_gate_set_vad_threshold(af_engine *e, double threshold);
int af_gate_set_hold_time(af_engine *e, double hold_ms);
int af_gate_set_margin(af_engine *e, double margin_db);
int af_gate_set_auto_threshold(af_engine *e, int32_t enabled);
int af_gate_read_vad_controls(const af_engine *e, double *vad_threshold, double *hold_ms, double *margin_db, int32_t *auto_threshold,
                              int32_t *attached);
int af_gate_set_vad_evidence(af_engine *e, const float *probabilities, const uint8_t *available, int64_t n_blocks, int32_t per_stream);
/* the decision rows of the last call that ran the fused path (synchronises), [block][stream]: the clamped probability, the
 * noise floor after the block's controller step, and flags (bit 0 held-open, bit 2 available) -- what
 * process_with_external_probability handed the per-sample loop (gate.rs:662-669).  n_blocks must be that call's block count. */
int af_engine_read_gate_vad_decisions(af_engine *e, float *probability, float *noise_floor_db, int32_t *flags, int64_t n_blocks);
int af_engine_read_gate_vad_state(af_engine *e, float *noise_floor_db, float *noise_floor_reliability, float *fused_score,
                                  float *probability, int32_t *gate_state, int32_t *flags, int32_t n_streams);

/* ---- RNNoise suppressor: rust-core/src/dsp/rnnoise.rs (RNNoiseProcessor) -------------------------
 * Runs between the front end and the EQ (dsp_loop.rs:1521-1599).  48 kHz only.  The suppressor eats whole
 * 480-sample frames: what a process call leaves over waits in the engine for the next call (rnnoise.rs:114-164), and a
 * call returns floor((pending + n) / 480) * 480 samples per stream (see af_engine_stream_host below).  Output is delayed by one frame
 * (latency_samples() = 480, rnnoise.rs:313-315).  The network weights of nnnoiseless 0.5.2 are not
 * available offline: engines start on seeded synthetic weights in the real layout; load the real
 * ones with af_suppressor_load_weights (blob = the model's fifteen int8 arrays: input_dense w,b;
 * vad_gru w,u,b; vad_output w,b; noise_gru w,u,b; denoise_gru w,u,b; denoise_output w,b). */
int af_engine_set_suppressor_enabled(af_engine *e, int32_t enabled);
int af_engine_set_suppressor_strength(af_engine *e, float strength);  /* rnnoise.rs:67-72, live */
int af_suppressor_set_synthetic_weights(af_engine *e, uint64_t seed);
int af_suppressor_load_weights(af_engine *e, const int8_t *blob, size_t bytes);
/* 1: the file protocol of bin/rnnoise_benchmark.rs:51-117 (clamp(+-1)*32768 in, /32768 out, no mix) */
int af_suppressor_set_raw_protocol(af_engine *e, int32_t enabled);
int32_t af_suppressor_latency_samples(const af_engine *e);
/* test tap: RNNoiseProcessor::scale_sample_for_model (rnnoise.rs:89-111; pinned by rnnoise.rs:335-352) evaluated
 * element-wise by the device function the pre-pass kernel uses; host pointers */
int af_suppressor_debug_scale_for_model(const float *in, float *out, int64_t n, int32_t device);
/* test tap: (silence flag, pitch index) of every frame of the last process call, [frame][stream][2] int32 */
int af_suppressor_set_trace_enabled(af_engine *e, int32_t enabled);
int64_t af_suppressor_trace_frames(const af_engine *e);
int af_suppressor_read_trace(af_engine *e, int32_t *out, int64_t capacity_frames);
/* test tap: the analysis record (158 floats/ints) and spectra X, P (481 complex each) of one
 * (frame, stream) cell of the suppressor's buffer set 0.  The windows of a call rotate through the
 * sets, so this is the call's last window only when the call had at most one window per set: valid
 * after a one-window call */
int af_suppressor_debug_read(af_engine *e, int32_t frame, int32_t stream, float *record, float *x_spectrum,
                             float *p_spectrum);
/* test tap of the pitch path (synchronises): the LPC-whitened, 2x-decimated pitch buffer (864 floats) of one (frame, stream)
 * cell of the last suppressor window (`whitened` null: skipped, `frame` ignored), and the stream's tracker state as the last
 * call left it: last_period, last_gain (null pointers are skipped).  AF_ERR_STATE before the first window,
 * AF_ERR_INVALID_ARGUMENT out of range; nothing is written then. */
int af_suppressor_debug_read_pitch(af_engine *e, int32_t frame, int32_t stream, float *whitened, int32_t *last_period,
                                   float *last_gain);
/* test tap of the pre-pass (synchronises): one stream's row of the last suppressor window's model-input buffer, i.e. the 1728
 * history samples the pre-pass put in front followed by the window's 480 x frames samples.  `*length` receives the row's
 * length; `row` (null: only the length is reported) must have room for it (`capacity` floats).  AF_ERR_STATE before the
 * first window, AF_ERR_INVALID_ARGUMENT out of range or too small; nothing is written then. */
int af_suppressor_debug_read_model_input(af_engine *e, int32_t stream, float *row, int64_t capacity, int64_t *length);
/* test tap: the pitch search kernel ALONE (decimation, whitening, coarse + fine search, interpolation offset), launched as the
 * engine launches it, on caller-supplied model-input spans [stream][1728 + 480 n_frames] (host pointers; frame f's pitch buffer
 * is span[480 (f + 1) .. 480 (f + 1) + 1728)).  Returns the whitened buffers [frame][stream][864] and the search's own pitch
 * index [frame][stream], which the tracker overwrites in an engine run.  n_streams in [1, 4096], n_frames in [1, 64]. */
int af_suppressor_debug_pitch_search(const float *spans, int32_t n_streams, int32_t n_frames, float *whitened,
                                     int32_t *pitch_index, int32_t device);

/* ---- ParametricEQ: rust-core/src/dsp/eq.rs --------------------------------------- */
int af_eq_set_band_frequency(af_engine *e, int32_t band, double frequency_hz); /* eq.rs:419-425 */
int af_eq_set_band_gain(af_engine *e, int32_t band, double gain_db);           /* eq.rs:406-412 */
int af_eq_set_band_q(af_engine *e, int32_t band, double q);                    /* eq.rs:432-438 */
int af_eq_set_band_config(af_engine *e, int32_t band, const af_eq_band_config *c); /* eq.rs:468-472 */
int af_eq_reset(af_engine *e);                                                 /* eq.rs:395-399 */
/* EqBandConfig::validate, eq.rs:140-201; message via af_last_error() */
int af_eq_band_config_validate(const af_eq_band_config *c, int32_t index, double sample_rate);

/* ---- Compressor: rust-core/src/dsp/compressor.rs:210-371 ------------------------ */
int af_compressor_set_threshold(af_engine *e, double threshold_db);
int af_compressor_set_ratio(af_engine *e, double ratio);
int af_compressor_set_attack_time(af_engine *e, double attack_ms);
int af_compressor_set_release_time(af_engine *e, double release_ms);
int af_compressor_set_makeup_gain(af_engine *e, double makeup_gain_db);
int af_compressor_set_adaptive_release(af_engine *e, int32_t enabled);
int af_compressor_set_base_release_time(af_engine *e, double release_ms);
int af_compressor_set_auto_makeup_enabled(af_engine *e, int32_t enabled);
int af_compressor_set_target_lufs(af_engine *e, double target_lufs);
int af_compressor_set_sidechain_highpass_enabled(af_engine *e, int32_t enabled);
int af_compressor_set_noise_reference_reliability(af_engine *e, double reliability); /* compressor.rs:351-353 */
/* AutoMakeupActivityInput (compressor.rs:32-37) for the NEXT af_engine_process_* call: one speech
 * posterior per control block (shared by all streams, or [block][stream] when per_stream != 0) plus
 * the three scalars simulate_auto_makeup_control passes (python_api.rs:211-219).  n_blocks = 0
 * clears the evidence (process_block_inplace without evidence, compressor.rs:695-697).  May be
 * called between process calls. */
int af_compressor_set_activity_evidence(af_engine *e, const double *vad_probabilities, int64_t n_blocks,
                                        int32_t per_stream, double vad_reliability, double noise_floor_db,
                                        double live_noise_reliability);

/* ---- Limiter: rust-core/src/dsp/limiter.rs:139-184 ------------------------------ */
int af_limiter_set_ceiling(af_engine *e, double ceiling_db);
int af_limiter_set_release_time(af_engine *e, double release_ms);
int af_limiter_set_lookahead_ms(af_engine *e, double lookahead_ms);
double af_limiter_ceiling_db(const af_engine *e);
int32_t af_limiter_lookahead_samples(const af_engine *e);

/* ---- TruePeakLimiter: rust-core/src/dsp/true_peak.rs:304-313 --------------------- */
int af_true_peak_limiter_set_release_ms(af_engine *e, float release_ms);

/* ---- DeEsser: rust-core/src/dsp/deesser.rs:288-353 ------------------------------ */
int af_deesser_set_auto_enabled(af_engine *e, int32_t enabled);
int af_deesser_set_auto_amount(af_engine *e, double amount);
int af_deesser_set_low_cut_hz(af_engine *e, double hz);
int af_deesser_set_high_cut_hz(af_engine *e, double hz);
int af_deesser_set_threshold_db(af_engine *e, double db);
int af_deesser_set_ratio(af_engine *e, double ratio);
int af_deesser_set_attack_ms(af_engine *e, double ms);
int af_deesser_set_release_ms(af_engine *e, double ms);
int af_deesser_set_max_reduction_db(af_engine *e, double db);

/* ---- processing ------------------------------------------------------------------ */
/* OfflineDspBlockProcessor::process_block_with_stats (block_processor.rs:106-161)
 * applied to every stream, for ceil(n/control_block) consecutive blocks.
 *
 * _device: `in`/`out` are device pointers on the engine's device; element (s, t) is at
 *   in[s*stream_stride + t] (stream-major) or in[t*stream_stride + s] (time-major);
 *   `hip_stream` is a hipStream_t (NULL = default stream).  Asynchronous: returns
 *   after enqueueing.  `in` may equal `out`.
 * _host: host pointers; copies in, runs, copies out, synchronises. */
int af_engine_process_device(af_engine *e, const float *in, float *out, int64_t n_samples,
                             int64_t stream_stride, int32_t layout, void *hip_stream);
int af_engine_process_host(af_engine *e, const float *in, float *out, int64_t n_samples,
                           int32_t layout);
int af_engine_synchronize(af_engine *e);
/* One wake-up of the realtime loop with the suppressor on (dsp_loop.rs:1521-1599: push_samples -> process_frames ->
 * pop_samples_into -> downstream chain): n_in new samples per stream go in ([stream][n_in]), the whole 480-sample frames
 * that are complete come out (*n_out = floor((pending + n_in) / 480) * 480 per stream at out_stride, possibly 0 or more
 * than n_in), the remainder waits in the engine.  af_engine_process_* follow the same rule (af_engine_process_device
 * needs stream_stride >= that count; af_engine_process_host fails when it exceeds n_samples).  Without the suppressor
 * *n_out == n_in.  Reference test: rnnoise.rs:355-370 (400 in -> 0 out, 400 pending; +100 -> 480 out, 20 pending). */
int af_engine_stream_host(af_engine *e, const float *in, int64_t n_in, float *out, int64_t out_stride, int64_t *n_out);
int64_t af_engine_pending_input(const af_engine *e);        /* RNNoiseProcessor::pending_input, rnnoise.rs:234-237 */
int64_t af_engine_last_output_samples(const af_engine *e);  /* samples per stream the last process call produced */
/* Blocks produced by the last process call and their stats, row-major [block][stream]
 * (synchronises).  `capacity` is in rows of af_block_stats. */
int64_t af_engine_last_block_count(const af_engine *e);
int af_engine_read_block_stats(af_engine *e, af_block_stats *out, int64_t capacity);
/* total samples per stream processed since create/reset */
int64_t af_engine_samples_processed(const af_engine *e);
/* ---- presets ---------------------------------------------------------------------
 * The reference configures one processor per stream (python/mic_eq/config_parts/settings.py:543-593).  An engine runs its
 * streams in groups of 64 (one chain workgroup each) and every group may run its own preset: add presets (each starts as a
 * fresh OfflineDspBlockProcessor::new, block_processor.rs:46-60), select the one the chain / EQ / compressor / limiter /
 * de-esser setters address, and map groups to presets (one index per 64 streams).  The control block, the front-end
 * switches, the suppressor and the kernel choice stay engine-wide.  Multi-preset engines run the plain token-ring form:
 * AF_ERR_UNSUPPORTED when a preset enables the de-esser or auto-makeup, or its limiter lookahead does not fit the ring. */
int af_engine_set_preset_count(af_engine *e, int32_t n);
int32_t af_engine_preset_count(const af_engine *e);  /* VALUE */
int af_engine_select_preset(af_engine *e, int32_t preset);
int af_engine_assign_presets(af_engine *e, const int32_t *preset_of_group, int32_t n_groups);
/* choose the kernel variant (AF_KERNEL_*); default AF_KERNEL_AUTO: up to 3072 streams (2048 behind the suppressor) AF_KERNEL_STAGED
 * (the chain as a pipeline of stage kernels, one per recurrence; not built for the de-esser, the front end without the
 * suppressor, more than 16 EQ sections, presets that differ in which stages run, time-major audio: those fall through); else AF_KERNEL_PHASED
 * (the token ring, 64 streams per workgroup) wherever its LDS layout fits, AF_KERNEL_QUAD (16 streams per workgroup) for
 * longer limiter lookaheads, AF_KERNEL_LANE_PER_STREAM otherwise.  The choice is made at the first process call after a
 * reset and kept (kernel 4 keeps its delay lines in buffers of its own).  All variants give the same bits. */
int af_engine_set_kernel(af_engine *e, int32_t kernel);
/* AF_KERNEL_* the most recent chain launch used; VALUE, not a status */
int af_engine_last_kernel(const af_engine *e);
/* test tap (synchronises): chunks, summed over the 64-stream groups of every token-ring launch of this engine so far, whose
 * output true-peak detector reused the maxima of the input observer instead of running its own FIR (same bits either way) */
int af_engine_debug_detector_reuse_chunks(af_engine *e, uint64_t *chunks);
/* tuning of the token-ring kernel: wavefronts per 64-stream group and samples per chunk
 * (built: 16x4, 16x2, 12x4, 12x2, 8x4, 8x2; 0,0 = default) */
int af_engine_set_ring_variant(af_engine *e, int32_t waves, int32_t chunk);
/* HIP-event timing of the kernels launched by the last process call, in milliseconds,
 * measured on the stream the kernels ran on (0 when timing is disabled) */
int af_engine_set_timing_enabled(af_engine *e, int32_t enabled);
int af_engine_last_kernel_ms(af_engine *e, double *ms, int32_t *launches);
/* the same split at the suppressor | chain boundary (front-end pre-pass counts as suppressor time) */
int af_engine_last_stage_ms(af_engine *e, double *suppressor_ms, double *chain_ms);
/* chain launches of the last call: their summed duration and the number of segments (`tail_ms` is always 0: it belonged
 * to a two-launch form of the chain that was measured slower and removed) */
int af_engine_last_chain_launch_ms(af_engine *e, double *first_ms, double *tail_ms, int32_t *segments);

/* ---- product resampler ------------------------------------------------------------------
 * `build_sinc_resampler_with_quality` + `simulate_product_resampler`
 * (rust-core/src/audio/processor/resampling.rs:140-156, 179-261): rubato's asynchronous windowed-sinc
 * resampler (sinc_len taps, 256 oversampled rows, cubic interpolation), driven in chunks of `chunk_size`
 * frames: full chunks, one zero-padded partial chunk, then silent flush chunks until expected + delay
 * frames exist.  One af_resampler serves any number of equally long f64 streams per call; audio is
 * stream-major ([stream][frame], strides in frames).  Windows: resampler_window_from_name,
 * resampling.rs:158-168. */
typedef struct af_resampler af_resampler;
enum { AF_WINDOW_BLACKMAN_HARRIS = 0, AF_WINDOW_BLACKMAN_HARRIS_SQUARED = 1, AF_WINDOW_BLACKMAN = 2,
       AF_WINDOW_BLACKMAN_SQUARED = 3, AF_WINDOW_HANN = 4, AF_WINDOW_HANN_SQUARED = 5 };
/* rubato::calculate_cutoff(sinc_len, window) (resampling.rs:149) */
int af_resampler_calculate_cutoff(int32_t sinc_len, int32_t window, float *out);
/* argument contract of resampling.rs:187-214 (AF_ERR_INVALID_ARGUMENT with the reference's messages);
 * AF_ERR_UNSUPPORTED when sinc_len / ratio need a longer input span than the kernel's LDS tile */
int af_resampler_create(uint32_t input_rate, uint32_t output_rate, int64_t chunk_size, int32_t sinc_len,
                        int32_t window, int32_t device, af_resampler **out);
void af_resampler_destroy(af_resampler *r);
/* Resampler::output_delay (resampling.rs:216); VALUE, not a status */
int af_resampler_output_delay(const af_resampler *r);
/* round(n_in * output_rate / input_rate) (resampling.rs:217-218); VALUE */
int64_t af_resampler_expected_frames(const af_resampler *r, int64_t n_in);
/* effective sinc length (rounded up to a multiple of 8 like the crate); VALUE */
int af_resampler_sinc_len(const af_resampler *r);
/* the 256 x sinc_len coefficient table, row-major (diagnostics / cross-checks) */
int af_resampler_copy_sinc_table(const af_resampler *r, double *out);
/* host only: frames the reference's driver loop returns for n_in input frames, and how many chunks it runs */
int af_resampler_plan(af_resampler *r, int64_t n_in, int64_t *n_out, int64_t *blocks);
/* all streams, all chunks, one launch; writes af_resampler_plan's n_out frames per stream */
int af_resampler_process_device(af_resampler *r, const double *d_in, double *d_out, int64_t n_in,
                                int32_t n_streams, int64_t in_stride, int64_t out_stride, void *hip_stream);
/* host buffers (checks "samples must be finite" -> AF_ERR_NON_FINITE) */
int af_resampler_process_host(af_resampler *r, const double *in, double *out, int64_t n_in, int32_t n_streams,
                              int64_t in_stride, int64_t out_stride);
/* HIP-event time of the last launch */
int af_resampler_last_kernel_ms(af_resampler *r, double *ms);
/* host only, touches no device: the kernel af_resampler_process_* launches for this resampler, chosen by the launcher's own
 * rule from the ratio, the sinc length and AF_RESAMPLER_VARIANT as read at create.  *form: 0 the vector body, 1 the
 * matrix-core body; *segment_outputs: output frames one workgroup takes (128, 64, 32, 16 or 8; always 128 for the
 * matrix-core body); *streams_per_workgroup: 64, or 32 for AF_RESAMPLER_VARIANT=mfma32.  Any pointer may be NULL. */
int af_resampler_launch_form(const af_resampler *r, int32_t *form, int32_t *segment_outputs,
                             int32_t *streams_per_workgroup);

/* ---- streaming product resampler -----------------------------------------------------------------
 * The same SincFixedIn as the realtime loop drives it (rust-core/src/audio/processor/dsp_loop.rs:274-317 builds one per
 * side whose device rate differs from the processing rate; :963-1011 input side, :843-895 output side): every wake-up
 * pushes its new f32 samples `as f64` into a queue, runs process_into_buffer while a whole chunk (input_frames_next() ==
 * chunk_size) is queued, takes the produced frames back `as f32`, and leaves the rest for the next wake-up.  An
 * af_stream_resampler is that object for `n_streams` streams advancing in lock step: positions, the queue length and the
 * chunk counter are host scalars, the audio state (2 * sinc_len frames of history + the queued remainder, f32) lives on
 * the device.  Audio is f32, stream-major, strides in frames.  No partial chunk, no flush: what af_resampler_* add for
 * whole clips is the offline driver's (resampling.rs:179-261), not the loop's. */
typedef struct af_stream_resampler af_stream_resampler;
/* build_sinc_resampler_with_quality (resampling.rs:140-156) with the argument contract and messages of
 * af_resampler_create (resampling.rs:187-214; AF_ERR_UNSUPPORTED beyond sinc_len 256 or below ratio 0.2: the LDS tile).
 * Every argument is validated before any HIP call; no GPU work happens until the first push. */
int af_stream_resampler_create(uint32_t input_rate, uint32_t output_rate, int64_t chunk_size, int32_t sinc_len,
                               int32_t window, int32_t n_streams, int32_t device, af_stream_resampler **out);
void af_stream_resampler_destroy(af_stream_resampler *r);
/* One wake-up (dsp_loop.rs:963-1011): appends n_in frames per stream (in[s * in_stride + t]), runs every chunk that is
 * complete, writes the frames they produce (rounded to f32, nearest even) to out[s * out_stride + t] and keeps the
 * remainder (< chunk_size frames).  *n_out = frames produced per stream, possibly 0.  Validated before anything is
 * touched: AF_ERR_INVALID_ARGUMENT when out_capacity (frames per stream `out` can take) or out_stride is below what the
 * call produces (af_stream_resampler_output_frames), AF_ERR_NON_FINITE "samples must be finite" (resampling.rs:206-210);
 * a refused call leaves the queue, the history and the position as they were.  Host pointers; synchronises. */
int af_stream_resampler_push_host(af_stream_resampler *r, const float *in, int64_t n_in, int64_t in_stride, float *out,
                                  int64_t out_capacity, int64_t out_stride, int64_t *n_out);
/* The same with device pointers, asynchronous on `hip_stream` (a hipStream_t, NULL = default stream): enqueues and returns,
 * never waits on the host (the per-call position table goes through pinned staging slots).  Successive pushes must be
 * ordered by the caller (one stream, or events).  FINITE INPUT IS THE CALLER'S CONTRACT here: nothing on the device
 * checks it.  Unlike the crate, whose dot products span exactly sinc_len frames, the kernels run every sinc row with
 * zero pad taps either side, and NaN * 0 = NaN: a non-finite frame would also reach the outputs whose windows merely
 * neighbour it. */
int af_stream_resampler_push_device(af_stream_resampler *r, const float *d_in, int64_t n_in, int64_t in_stride,
                                    float *d_out, int64_t out_capacity, int64_t out_stride, int64_t *n_out,
                                    void *hip_stream);
/* frames per stream the next push of n_in frames would produce: a host replay of process_into_buffer's position loop,
 * changes no state; VALUE */
int64_t af_stream_resampler_output_frames(const af_stream_resampler *r, int64_t n_in);
/* resample_input.len() after the last push (dsp_loop.rs:984); VALUE */
int64_t af_stream_resampler_pending_input(const af_stream_resampler *r);
/* Resampler::output_delay (resampling.rs:216); VALUE */
int af_stream_resampler_output_delay(const af_stream_resampler *r);
/* frames per stream pushed / produced since create or reset; VALUES */
int64_t af_stream_resampler_frames_in(const af_stream_resampler *r);
int64_t af_stream_resampler_frames_out(const af_stream_resampler *r);
/* a fresh resampler (what dsp_loop.rs:274-317 builds at start): zero history, position -sinc_len / 2, nothing queued */
int af_stream_resampler_reset(af_stream_resampler *r);
/* the input backlog drop, dsp_loop.rs:941-944 (resample_input.clear()): the queue is emptied, history and position stay */
int af_stream_resampler_clear_pending(af_stream_resampler *r);
/* HIP-event time of the last push's kernels */
int af_stream_resampler_last_kernel_ms(af_stream_resampler *r, double *ms);
/* as af_resampler_launch_form, for the kernel a push launches */
int af_stream_resampler_launch_form(const af_stream_resampler *r, int32_t *form, int32_t *segment_outputs,
                                    int32_t *streams_per_workgroup);

/* ---- device-rate I/O of an engine: dsp_loop.rs:274-317 ---------------------------------------------------------
 * af_engine_set_io_sample_rates: a configuration setter (AF_ERR_STATE after streaming started).  A rate of 0, or equal to
 *   the engine's, means no resampler on that side (dsp_loop.rs:274, 292); with both sides off every call behaves as
 *   without this setter.  Otherwise that side gets build_sinc_resampler's product configuration (resampling.rs:140-156).
 * With a rate set, af_engine_stream_host takes `in` at the input rate and returns `out` at the output rate: input
 *   resampler (dsp_loop.rs:963-1011) -> the chain on the frames it produced (not called when no chunk completed) -> output
 *   resampler (dsp_loop.rs:843-895; not called when the chain returned nothing).  *n_out is what af_engine_stream_plan
 *   said; out_stride below it refuses the call with everything untouched.  af_engine_process_host / _device return
 *   AF_ERR_UNSUPPORTED.  af_engine_reset restarts both resamplers.  Block statistics, af_engine_samples_processed,
 *   af_engine_pending_input and the evidence setters stay in engine-rate samples: size evidence from
 *   af_engine_stream_plan's engine_frames_*.
 *   DEVIATION: a non-finite host sample refuses the call (AF_ERR_NON_FINITE, nothing touched).  The reference resamples
 *   first and scrubs afterwards (routing.rs:802-823), which smears one NaN over the 2 * sinc_len frames around it and
 *   then zeroes them all.
 * af_engine_stream_plan: exact host replay, changes no state: the frames the input resampler will hand the chain, the
 *   frames the chain will return (the suppressor's 480-frame rule included) and the frames that will come out.
 * af_engine_io_resampler_delay: output_delay() of each side, 0 when off; the loop adds the output side's to its
 *   reported latency (dsp_loop.rs:310-313).
 * af_engine_io_resampler_pending: frames queued in each side's resampler (af_stream_resampler_pending_input), 0 when off. */
int af_engine_set_io_sample_rates(af_engine *e, uint32_t input_rate, uint32_t output_rate);
int af_engine_stream_plan(const af_engine *e, int64_t n_in, int64_t *engine_frames_in, int64_t *engine_frames_out,
                          int64_t *n_out);
int af_engine_io_resampler_delay(const af_engine *e, int32_t *input_frames, int32_t *output_frames);
int af_engine_io_resampler_pending(const af_engine *e, int64_t *input_frames, int64_t *output_frames);

/* ---- input mixdown: multichannel device frames -> mono ----------------------------------------------------------
 * What the reference's capture callback does before a frame reaches the input ring (rust-core/src/audio/input.rs:785-843
 * over :383-736): interleaved frames of `n_channels` channels become mono under one of five InputChannelModes
 * (input.rs:137-144): 0 average, 1 left, 2 right, 3 max_rms (the channel with the largest energy of the chunk,
 * input.rs:383-407), 4 phase_safe_mono.  For stereo, phase_safe_mono measures the channel correlation (input.rs:409-435),
 * searches 17 lags x 2 polarities for a better alignment and refines the lag with a parabola (input.rs:477-537), then mixes
 * by a polarity flip, a 4-point Lagrange fractional delay (input.rs:121-134), the strongest channel or a plain average, with
 * a hysteresis on the decision and a 16-frame history across callbacks (input.rs:539-636).  Off stereo it is the average
 * (input.rs:719).  One channel is a copy (input.rs:789-805).  A call is one callback: it is cut into chunks of at most 8192
 * frames with one decision each (input.rs:807-842).  An af_mixdown is that for `n_streams` independent streams; the result
 * is bit-exact with the reference's f32 arithmetic.  f32 frames only: the reference converts i16 / u16 device formats
 * through cpal first.  Audio layout: in[(s * in_stride_frames + t) * n_channels + c], out[s * out_stride + t]. */
typedef struct af_mixdown af_mixdown;
/* Everything is validated before any HIP call: n_channels >= 1 (AF_ERR_UNSUPPORTED above 8), mode 0..4 (an unknown value
 * is refused: the reference's unwrap_or(Average), input.rs:815-816, guards a corrupted atomic, not an API), n_streams > 0.
 * No GPU work happens until the first push. */
int af_mixdown_create(int32_t n_channels, int32_t mode, int32_t n_streams, int32_t device, af_mixdown **out);
void af_mixdown_destroy(af_mixdown *m);
/* The mode is live: the callback loads it per chunk (input.rs:814-816), so a set takes effect with the next push and keeps
 * the history and last_candidate (input.rs:780 builds the state once per stream).  af_mixdown_mode / _channels: VALUES */
int af_mixdown_set_mode(af_mixdown *m, int32_t mode);
int32_t af_mixdown_mode(const af_mixdown *m);
int32_t af_mixdown_channels(const af_mixdown *m);
/* One callback of n_frames frames per stream, host pointers; synchronises.  DEVIATION: a non-finite sample refuses the call
 * with nothing touched (AF_ERR_NON_FINITE "samples must be finite"), as af_stream_resampler_push_host does; the reference
 * mixes whatever the device delivers (input.rs:785-843) and scrubs later (routing.rs:802-823). */
int af_mixdown_push_host(af_mixdown *m, const float *in, int64_t n_frames, int64_t in_stride_frames, float *out,
                         int64_t out_stride);
/* The same with device pointers, asynchronous on `hip_stream` (a hipStream_t, NULL = default stream): two launches per
 * chunk, no host wait.  Successive pushes must be ordered by the caller.  Finite input is the caller's contract. */
int af_mixdown_push_device(af_mixdown *m, const float *d_in, int64_t n_frames, int64_t in_stride_frames, float *d_out,
                           int64_t out_stride, void *hip_stream);
/* InputStreamOptions' atomics as the callback leaves them (input.rs:181-186, 825-838), one entry per stream, any pointer
 * may be null: the last Some stereo correlation (NaN until a first one), the count of chunks whose correlation was below
 * -0.75 (input.rs:24), and the last chunk's PhaseRescueStrategy (input.rs:31-37: 0 none, 1 polarity_flip,
 * 2 fractional_delay, 3 max_rms_fallback), estimated delay in frames and polarity-flipped flag.  Waits for the device. */
int af_mixdown_read_diagnostics(af_mixdown *m, float *stereo_correlation, uint64_t *phase_warning_count, int32_t *strategy,
                                float *estimated_delay, int32_t *polarity_flipped, int32_t n_streams);
/* a fresh PhaseSafeMonoState (input.rs:96-105) and fresh diagnostics: what a new input stream starts from (input.rs:780) */
int af_mixdown_reset(af_mixdown *m);
/* HIP-event times of the last push, summed over its chunks: the decision passes and the mix passes */
int af_mixdown_last_kernel_ms(af_mixdown *m, double *decision_ms, double *mix_ms);

/* ---- output writer: drift retime, discontinuity fade, safety limiter, queue accounting per stream ------------------
 * What the reference does to every block between the chain / output resampler and the playback queue
 * (rust-core/src/audio/processor/output_writer.rs:62-110, OutputWriteContext::write_chunk): the jitter-buffer retime
 * (:112-159 over resampling.rs:81-120), the fade after a short write (:161-192), scrub + a second TruePeakLimiter at the
 * device rate + ceiling clamp with clip metrics + a TruePeakDetector (:194-288, routing.rs:651-655, 697-703, 768-799) and
 * the queue write's accounting (:290-343).  An af_output_writer is that for `n_streams` independent streams.  The queue
 * itself is the caller's: each push is told how many frames every stream's queue holds (`fill`, capacity - free_len at
 * :67-69) and answers with how many frames of the row reach it (`written`, min(pending, free)).  The output is ragged:
 * stream s yields written[s] frames.  Audio, decisions, counters and linear statistics are bit-exact with the reference's
 * f32 arithmetic; the dB fields are 20 log10f of such values.  Layout: in[s * in_stride + t], out[s * out_stride + t]. */
typedef struct af_output_writer af_output_writer;
typedef struct af_output_writer_config {
  int32_t output_rate;      /* the limiter's rate: TruePeakLimiter::default_settings(output_rate), dsp_loop.rs:798-799 */
  int64_t queue_capacity;   /* frames the queue holds, dsp_loop.rs:204 */
  int64_t target_center;    /* OutputWriteLimits::output_target_center_samples, output_writer.rs:22 */
  int64_t hard_backlog;     /* ... output_hard_backlog_samples, :23 */
  int64_t fade_frames;      /* ... discontinuity_fade_samples, :24 */
} af_output_writer_config;
/* dsp_loop.rs:781-795 from the output rate: capacity 2 * rate (:204), centre div_ceil(30 ms + 40 ms, 2), hard backlog
 * 60 ms, fade max(6 ms, 1), each through duration_samples (resampling.rs:1-3).  The ratios are the reference's constants
 * (1.03 and 1.06, dsp_loop.rs:790-791; 0.008 and 0.96, processor.rs:69-70). */
int af_output_writer_default_config(int32_t output_rate, af_output_writer_config *cfg);
/* Everything is validated before any HIP call: rate > 0, capacity >= 1 and below 2^31, centre / backlog >= 0 and below
 * 2^31, fade 1 .. 2^31 - 1, 0 < n_streams <= 65535.  The limiter starts enabled with ceiling 1.0.  No GPU work happens
 * until the first push. */
int af_output_writer_create(const af_output_writer_config *cfg, int32_t n_streams, int32_t device, af_output_writer **out);
void af_output_writer_destroy(af_output_writer *w);
/* limiter_enabled and output_ceiling_linear are live: read at each push (output_writer.rs:208-215).  Disabled, the ceiling
 * is 1.0, the limiter is reset by every push, the gain-reduction field is 0 and its history decays by 0.15 (:219-227). */
int af_output_writer_set_limiter(af_output_writer *w, int32_t enabled, float ceiling_linear);
/* fresh EMA, fade, limiter, detector, counters and dB fields, as the loop builds them (dsp_loop.rs:796-802) */
int af_output_writer_reset(af_output_writer *w);
/* the longest row a push of n_in frames can yield: n_in on the clean path, round(n_in / 0.96) capped by the queue capacity
 * and the reference's 8672-frame scratch on the retimed one (resampling.rs:92-94).  VALUE; 0 for a null writer or n_in < 1 */
int64_t af_output_writer_max_output_frames(const af_output_writer *w, int64_t n_in);
/* One write_chunk per stream on host pointers; synchronises.  fill[s]: frames in stream s's queue at the call.  Row s of
 * `out` gets written[s] frames; the rest of the row is left untouched.  clean_path (the raw-monitor route,
 * routing.rs:691-694) skips the retime and the fade, not the safety step.  Validated before anything is touched: n_in == 0
 * is a no-op (the reference returns false, :63-65) that zeroes `written`; n_in > 8192, out_capacity or out_stride below
 * af_output_writer_max_output_frames(w, n_in), in_stride < n_in, or any fill[s] outside 0 .. capacity is
 * AF_ERR_INVALID_ARGUMENT.  DEVIATION: the reference's 8672-frame scratches truncate a longer block and raise
 * FixedBufferOverflow (:174-177, 204-207); here such a call is refused with nothing touched.  Non-finite input is
 * accepted: scrubbing it is this stage's job (:213). */
int af_output_writer_push_host(af_output_writer *w, const float *in, int64_t n_in, int64_t in_stride, const int64_t *fill,
                               int32_t clean_path, float *out, int64_t out_capacity, int64_t out_stride, int64_t *written);
/* The same with device pointers (fill and written too), asynchronous on `hip_stream` (a hipStream_t, NULL = default
 * stream): four or five launches whatever the data, no host wait.  Successive pushes must be ordered by the caller.  A
 * fill outside 0 .. capacity cannot be seen from the host: it is clamped on the device.  The first push allocates the writer's
 * scratch rows for the longest block (8192 frames in); no later push allocates or waits. */
int af_output_writer_push_device(af_output_writer *w, const float *d_in, int64_t n_in, int64_t in_stride, const int64_t *d_fill,
                                 int32_t clean_path, float *d_out, int64_t out_capacity, int64_t out_stride, int64_t *d_written,
                                 void *hip_stream);
/* OutputWriteCounters' running counts (output_writer.rs:2-5, 10, 12), one entry per stream, any pointer may be null.
 * Waits for the device. */
int af_output_writer_read_counters(af_output_writer *w, uint64_t *jitter_dropped, uint64_t *retime_adjustments,
                                   uint64_t *recovery_events, uint64_t *short_write_dropped, uint64_t *clip_events,
                                   uint64_t *true_peak_events, int32_t n_streams);
/* db: [6][n_streams], the atomics of output_writer.rs:11-17 in that order (clip peak, true peak, true-peak input, gain
 * reduction, gain-reduction history, headroom).  linear: [5][n_streams], the last push's input true peak, limiter output
 * true peak, detector true peak, minimum gain and maximum clipped amplitude.  Then the last push's ratio, the drift EMA,
 * out_len, the fade frames remaining and the modelled fill after the write (:333-343).  Any pointer may be null. */
int af_output_writer_read_meters(af_output_writer *w, float *db, float *linear, float *ratio, float *drift_ema, int64_t *out_len,
                                 int64_t *fade_remaining, int64_t *fill_after, int32_t n_streams);
/* test read-out of the limiter and detector state (true_peak.rs:250-263, 190-193): gain [n], the delay line [n][20] as the
 * reference indexes it, its write index [n], and the histories [n][3][32] (limiter input, limiter output, detector) */
int af_output_writer_read_state(af_output_writer *w, float *gain, float *delay, int32_t *write_idx, float *histories,
                                int32_t n_streams);
/* HIP-event time of the last push, all passes */
int af_output_writer_last_kernel_ms(af_output_writer *w, double *ms);
/* ... and of each pass: pass_ms[5] = plan, shape, gain (0 with the limiter off), out, finish */
int af_output_writer_last_pass_ms(af_output_writer *w, double *pass_ms);

/* ---- the output writer of an engine: dsp_loop.rs:781-895 ---------------------------------------------------------------
 * af_engine_set_output_writer: a configuration setter (AF_ERR_STATE after streaming started).  Enabled, every
 *   af_engine_stream_host call ends with one write_chunk per stream (output_writer.rs:62-110) on the device, behind the output
 *   resampler if one is set (then at the I/O output rate, otherwise at the engine's; limits as af_output_writer_default_config).
 *   limiter_enabled and the ceiling are the engine's limiter's, 10^(ceiling_db / 20) in f32 (dsp_loop.rs:535,
 *   output_writer.rs:208-215).  *n_out is the largest written[s]; rows are zero beyond their own length;
 *   af_engine_stream_plan's n_out becomes af_output_writer_max_output_frames of what it reported before, and out_stride must
 *   cover it.  A call whose output side exceeds 8192 frames is refused with everything untouched.  af_engine_process_host /
 *   _device return AF_ERR_UNSUPPORTED.  af_engine_reset resets the writer and drops the fill.  Disabled (the default), every
 *   call takes the branch it took before.
 * af_engine_set_output_queue_fill: fill[s] frames are in stream s's playback queue (capacity - free_len, output_writer.rs:67-69);
 *   used by every af_engine_stream_host from the next one until it is set again.  Until it is first set the fill is the target
 *   centre (no error, ratio 1).  0 .. capacity, AF_ERR_STATE with the writer off.
 * af_engine_read_output_written: written[s] of the last af_engine_stream_host.
 * af_engine_read_output_counters / _meters: as af_output_writer_read_counters / _meters. */
int af_engine_set_output_writer(af_engine *e, int32_t enabled);
int af_engine_set_output_queue_fill(af_engine *e, const int64_t *fill, int32_t n_streams);
int af_engine_read_output_written(af_engine *e, int64_t *written, int32_t n_streams);
int af_engine_read_output_counters(af_engine *e, uint64_t *jitter_dropped, uint64_t *retime_adjustments, uint64_t *recovery_events,
                                   uint64_t *short_write_dropped, uint64_t *clip_events, uint64_t *true_peak_events,
                                   int32_t n_streams);
int af_engine_read_output_meters(af_engine *e, float *db, float *linear, float *ratio, float *drift_ema, int64_t *out_len,
                                 int64_t *fade_remaining, int64_t *fill_after, int32_t n_streams);

/* ---- multichannel input of an engine: input.rs:785-843 ----------------------------------------------------------
 * af_engine_set_input_channels: a configuration setter (AF_ERR_STATE after streaming started), arguments as
 *   af_mixdown_create.  One channel means the feature is off and every call behaves as without this setter.  With more,
 *   af_engine_stream_host takes in[(s * n_in + t) * n_channels + c]; the mixdown runs first on the device and feeds the
 *   input resampler if one is set (dsp_loop.rs:963-1011), otherwise the chain.  af_engine_stream_plan keeps counting
 *   frames.  af_engine_process_host / _device return AF_ERR_UNSUPPORTED.  af_engine_reset resets the mixdown.
 * af_engine_set_input_channel_mode: live, as af_mixdown_set_mode (input.rs:814-816).
 * af_engine_read_input_phase: as af_mixdown_read_diagnostics; with one channel NaN / 0 / none / 0 / false (input.rs:789-793). */
int af_engine_set_input_channels(af_engine *e, int32_t n_channels, int32_t mode);
int af_engine_set_input_channel_mode(af_engine *e, int32_t mode);
int af_engine_read_input_phase(af_engine *e, float *stereo_correlation, uint64_t *phase_warning_count, int32_t *strategy,
                               float *estimated_delay, int32_t *polarity_flipped, int32_t n_streams);

/* ---- noise gate -------------------------------------------------------------------------------
 * NoiseGate (rust-core/src/dsp/gate.rs) on the path `simulate_gate_suppressor_order` exercises
 * (python_api.rs:312-319 builds the gate without a VadAutoGate, so process_block_inplace runs the per-sample
 * downward expander, gate.rs:626-637).  One-shot over whole clips from the initial state (gate.rs:158-225);
 * `vad_mode` != 0 = GateMode::VadAssisted/VadOnly (arms the chatter auto-relax, gate.rs:598-601).
 * gain_trace: [ceil(n / trace_block)][n_streams] `current_gain()` at the end of every block (python_api.rs:356);
 * chatter_events: [n_streams] `chatter_event_count()`.  Either may be null. */
int af_gate_process_host(const float *in, float *out, int64_t n_samples, int32_t n_streams, int64_t stream_stride,
                         double threshold_db, double attack_ms, double release_ms, double sample_rate,
                         int32_t vad_mode, int32_t trace_block, float *gain_trace, uint64_t *chatter_events,
                         int32_t device);

/* ---- integrated loudness ------------------------------------------------------------------
 * measure_integrated_loudness (rust-core/src/lib.rs:290-298 over dsp/loudness.rs:43-83): BS.1770 gated loudness of
 * whole clips, ebur128 `Mode::I | Mode::HISTOGRAM`, mono.  One value per stream; `status` (optional, [n_streams])
 * holds AF_OK, AF_ERR_NON_FINITE ("samples must be finite") or AF_ERR_UNSUPPORTED (nothing passed the gates:
 * "audio did not produce a finite gated loudness"); the call returns the first failure.  Sample rates:
 * loudness.rs:36-41. */
int af_measure_integrated_loudness_device(const float *d_audio, int64_t n_samples, int32_t n_streams,
                                          int64_t stream_stride, uint32_t sample_rate, int32_t device,
                                          double *lufs, int32_t *status);
int af_measure_integrated_loudness_host(const float *audio, int64_t n_samples, int32_t n_streams,
                                        int64_t stream_stride, uint32_t sample_rate, int32_t device,
                                        double *lufs, int32_t *status);

/* ---- voice spectrum measurement: python/mic_eq/analysis/spectrum.py ----------------------------------------------
 * The measurement behind every EQ preset, for a batch of captures: frame energies, voiced-frame selection (optionally fused
 * with a VAD posterior), Hamming-windowed spectra, the Welch spectrum over the voiced material, median speech and noise
 * spectra, per-bin SNR and the perceptual smoothing of every voiced window.  In scope: spectrum.py:69-343, 519-645 (up to
 * and including the single-spectrum fallback return) and 839-967 with strength "balanced".  Deviations: nperseg is a power of
 * two from 256 to 8192 (anything else: AF_ERR_UNSUPPORTED); non-finite audio is refused with AF_ERR_NON_FINITE.
 * Frames are nperseg samples at hop nperseg / 2; bins = nperseg / 2 + 1 at k * sample_rate / nperseg Hz. */
typedef struct af_voice_spectrum af_voice_spectrum;
enum { AF_NOISE_REFERENCE_UNAVAILABLE = 0, AF_NOISE_REFERENCE_EXPLICIT_CAPTURE = 1, AF_NOISE_REFERENCE_IN_CAPTURE_NON_SPEECH = 2,
       AF_NOISE_REFERENCE_VALIDATED_CONSERVATIVE = 3 };
/* one stream's scalars of analyze_voice_spectrum, spectrum.py:527-550, 570-586, 605, 625 */
typedef struct af_voice_spectrum_row {
  int32_t frames;                        /* (n_samples - nperseg) / hop + 1 */
  int32_t voiced;                        /* frames _voiced_frame_mask kept, :200-247 */
  double voiced_window_ratio;            /* :543; on the fallback branch max(ratio, 1 / frames), :625 */
  double vad_active_window_ratio;        /* :545-549 */
  int32_t vad_probability_used;          /* :550 */
  int32_t noise_reference_source;        /* AF_NOISE_REFERENCE_*, :553-586 */
  int32_t used_single_spectrum_fallback; /* :605 */
  int32_t welch_segments;                /* segments signal.welch averaged over what _select_voiced_samples kept, :69-107 */
} af_voice_spectrum_row;
/* Where a call writes; every pointer is host memory and may be null.  Spectra are [n_streams][bins] in dB. */
typedef struct af_voice_spectrum_outputs {
  af_voice_spectrum_row *rows;  /* [n_streams] */
  double *speech_db;            /* _median_frame_spectrum_db of the voiced frames, :551; NaN row where it is None */
  double *noise_db;             /* the noise reference on the same grid, :596-602; NaN row where it is None */
  double *spectral_snr_db;      /* _spectral_snr_db, :333-342, :603; NaN row where it is None */
  double *welch_db;             /* compute_voice_spectrum, :110-164 */
  double *welch_sum;            /* its sum over segments of |X|^2, before scaling */
  double *frame_power;          /* [n_streams][frames] mean of x^2 */
  double *frame_rms_db;         /* [n_streams][frames] _frame_rms_db, :167-169 */
  uint8_t *voiced_mask;         /* [n_streams][frames] */
  int32_t keep_windows;         /* != 0: smooth the voiced frames' spectra and keep them for af_voice_spectrum_read_windows
                                   (host memory: voiced frames x bins x 3 doubles over the whole batch) */
} af_voice_spectrum_outputs;
int af_voice_spectrum_create(uint32_t sample_rate, int32_t nperseg, int32_t device, af_voice_spectrum **out);
void af_voice_spectrum_destroy(af_voice_spectrum *h);
int32_t af_voice_spectrum_bins(const af_voice_spectrum *h);                       /* VALUE */
int64_t af_voice_spectrum_frames(const af_voice_spectrum *h, int64_t n_samples);  /* VALUE: 0 below nperseg */
/* get_octave_frequencies(fraction), default limits and reference, :839-889.  *n_bands is always set. */
int af_voice_spectrum_octave_bands(int32_t fraction, double *centre, double *lower, double *upper, int32_t capacity, int32_t *n_bands);
/* analyze_voice_spectrum :519-645 and compute_voice_spectrum :110-164 for audio[n_streams][stride]; n_samples below nperseg
 * is refused with the reference's "Audio too short for FFT" text.  vad_probabilities: null, or [n_streams][n_vad] posteriors
 * per 32 ms model window (:172-197).  noise_audio: null, or [n_streams][noise_stride] room-noise captures of n_noise samples
 * (:570-577; below nperseg it is ignored, :326-327).  _host takes host audio, _device device audio (on the null stream);
 * both return after the outputs are written. */
int af_voice_spectrum_analyze_host(af_voice_spectrum *h, const float *audio, int64_t n_samples, int32_t n_streams, int64_t stride,
                                   const double *vad_probabilities, int64_t n_vad, const float *noise_audio, int64_t n_noise,
                                   int64_t noise_stride, const af_voice_spectrum_outputs *out);
int af_voice_spectrum_analyze_device(af_voice_spectrum *h, const float *d_audio, int64_t n_samples, int32_t n_streams, int64_t stride,
                                     const double *vad_probabilities, int64_t n_vad, const float *d_noise_audio, int64_t n_noise,
                                     int64_t noise_stride, const af_voice_spectrum_outputs *out);
/* The voiced frames of one stream of the last call with keep_windows, in frame order, [frames][bins]: _window_spectrum_db
 * (:293-300), smooth_spectrum_perceptual of it (:949-967) and the PSD before the dB.  *n_frames is set whenever the call
 * succeeds; with all three arrays null it only counts.  AF_ERR_STATE when the last call kept nothing. */
int af_voice_spectrum_read_windows(af_voice_spectrum *h, int32_t stream, double *raw_db, double *smoothed_db, double *linear_psd,
                                   int32_t max_frames, int32_t *n_frames);
/* GPU time of the kernels of the last call (events around them; copies and host decisions are not in it) */
int af_voice_spectrum_last_kernel_ms(af_voice_spectrum *h, double *ms);
/* The second half of analyze_voice_spectrum, spectrum.py:647-742 with _robust_median_spectrum (:250-290) and
 * _measurement_reliability (:381-495): opt-in and off by default; with it off no call changes by a bit.  With it on, an
 * analyze call also smooths the voiced windows of every stream that does not take the fallback (keep_windows or not; the
 * rows stay on the device) and keeps the results below for af_voice_spectrum_read_reliability. */
int af_voice_spectrum_set_reliability(af_voice_spectrum *h, int32_t enabled);
/* one stream's scalars of the main branch's return, :722-742; on the fallback branch the constants of :620-644 */
typedef struct af_voice_spectrum_reliability_row {
  double snr_db;                        /* _estimate_snr_from_spectrum of the robust median, :673 (:626 of Welch on the fallback) */
  double spectral_tilt_db_per_octave;   /* _estimate_tilt_db_per_octave, :729 (:632) */
  double residual_confidence;           /* :701-721 (0, :633) */
  double measurement_coverage;          /* :692-700 (0.45, :635) */
  double outlier_rejection_ratio;       /* 1 - inlier ratio, :733 (0, :636) */
  double phonetic_coverage;             /* :480-488, :740 (0, :643) */
  double effective_measurement_blocks;  /* _effective_block_count, :411-424, :741 (0, :644) */
  int32_t voiced;                       /* windows the statistics saw (0 on the fallback) */
  int32_t independent;                  /* non-overlapping windows kept by :446-454 */
  int32_t blocks;                       /* block rows of :456-463 */
  int32_t inliers;                      /* windows behind the robust median, :279-285 */
  int32_t used_closest_windows;         /* the argsort branch of :281-285 was taken */
  int32_t reserved;
} af_voice_spectrum_reliability_row;
/* Where af_voice_spectrum_read_reliability writes; host memory, every pointer may be null.  Spectra are [n_streams][bins]. */
typedef struct af_voice_spectrum_reliability_outputs {
  af_voice_spectrum_reliability_row *rows;  /* [n_streams] */
  double *median_spectrum_db;          /* _robust_median_spectrum, :669, :724 (the Welch spectrum on the fallback, :623) */
  double *spectral_repeatability;      /* :478, :490, :728 (zeros, :620) */
  double *measurement_uncertainty_db;  /* :475-477, :739; +inf below two blocks (:467) and on the fallback (:642) */
  double *spectral_snr_db;             /* _spectral_snr_db of the robust median, :672 (:616 on the fallback); NaN row where None */
  double *window_distance;             /* [n_streams][frames] the shape distances of :275 at the voiced frames, NaN elsewhere */
  uint8_t *inlier_mask;                /* [n_streams][frames] 1 at the voiced frames :279-285 kept */
} af_voice_spectrum_reliability_outputs;
/* The reliability results of the last analyze call.  AF_ERR_STATE when that call ran with the option off or no call was made. */
int af_voice_spectrum_read_reliability(af_voice_spectrum *h, const af_voice_spectrum_reliability_outputs *out);
/* GPU time of the reliability kernels of the last call, summed over its tiles (they are part of
 * af_voice_spectrum_last_kernel_ms): ms[0 .. 5) = row levels, block and centre medians, shape distances, block statistics,
 * robust median.  Zeros when the option was off.  capacity: the doubles ms holds, at least 5. */
int af_voice_spectrum_last_reliability_kernel_ms(af_voice_spectrum *h, double *ms, int32_t capacity);
/* noise_spectrum_override of analyze_voice_spectrum, spectrum.py:554-569: a prevalidated noise spectrum (the conservative
 * spectrum of af_noise_reference_analyze_*) on its own grid freqs[n_points] (increasing), spectrum_db[n_streams][stride] dB,
 * or with shared != 0 one spectrum_db[n_points] for every stream; the arrays are copied.  spectrum_db null clears it.  While
 * it is set, an analyze call validates each stream's override as :557-563 does (at least 2 points, all finite): a valid one
 * takes precedence over noise_audio and the in-capture fallback, is interpolated onto the handle's grid with held ends
 * (:596-602) and reports AF_NOISE_REFERENCE_VALIDATED_CONSERVATIVE; an invalid one falls through silently.  A per-stream
 * override whose n_streams differs from the call's is AF_ERR_INVALID_ARGUMENT.  With none set no call changes by a bit. */
int af_voice_spectrum_set_noise_override(af_voice_spectrum *h, const double *freqs, const double *spectrum_db, int32_t n_points,
                                         int32_t n_streams, int64_t stride, int32_t shared);

/* smooth_spectrum_perceptual "balanced" (spectrum.py:949-967) of n_rows host spectra rows_db[n_rows][bins] (dB, on the handle's
 * grid) into out[n_rows][bins] (host): the pass every voiced window goes through, for spectra of the caller's -- the median
 * spectrum that the voice-chain recommendation reads (voice_setup.py:1163-1166).  Returns after out is written. */
int af_voice_spectrum_smooth_rows(af_voice_spectrum *h, const double *rows_db, int32_t n_rows, double *out);

/* ---- room-noise reference analysis: python/mic_eq/analysis/noise_reference.py:118-546 ------------------------------
 * analyze_noise_reference for a batch of capture pairs: the quality verdict on a room-tone capture (duration, finiteness,
 * silence, clipping, stationarity, transients, speech contamination, metadata, age, consistency with the quiet frames of the
 * voice capture) and the explicit, in-capture and conservative noise spectra.  Frames are max(512, round(0.2 sample_rate))
 * samples at half that hop, Hann-windowed.  The frame must be even, its half free of prime factors above 7 and at most 10240
 * (8, 12, 16, 22.05, 24, 32, 44.1, 48, 64, 88.2, 96 kHz and everything up to 2.56 kHz qualify; anything else:
 * AF_ERR_UNSUPPORTED at create).  A non-finite sample reads as 0 and makes its capture invalid, as in the reference. */
typedef struct af_noise_reference af_noise_reference;
enum { AF_NOISE_STATUS_USABLE = 0, AF_NOISE_STATUS_QUESTIONABLE = 1, AF_NOISE_STATUS_INVALID = 2 };
/* bits of af_noise_reference_row.reasons, one per distinct text of :315-470, in the order the reference appends them */
enum {
  AF_NOISE_REASON_TOO_SHORT = 1u << 0,            /* "room-noise capture is too short" */
  AF_NOISE_REASON_NON_FINITE = 1u << 1,           /* "... contains non-finite samples" */
  AF_NOISE_REASON_SILENT = 1u << 2,               /* "... is suspiciously silent" */
  AF_NOISE_REASON_CLIPPED = 1u << 3,              /* "... is clipped" */
  AF_NOISE_REASON_ISOLATED_CLIPS = 1u << 4,       /* "... contains isolated clipped samples" */
  AF_NOISE_REASON_TOO_FEW_WINDOWS = 1u << 5,      /* "... has too few analysis windows" */
  AF_NOISE_REASON_CHANGING_EVENTS = 1u << 6,      /* "... is dominated by changing events" */
  AF_NOISE_REASON_NOT_STATIONARY = 1u << 7,       /* "... is not stationary" */
  AF_NOISE_REASON_DOMINANT_TRANSIENTS = 1u << 8,  /* "... contains dominant transient events" */
  AF_NOISE_REASON_STRONG_TRANSIENTS = 1u << 9,    /* "... contains strong transients" */
  AF_NOISE_REASON_SPEECH_PRESENT = 1u << 10,      /* "speech is present in the room-noise capture" */
  AF_NOISE_REASON_POSSIBLE_SPEECH = 1u << 11,     /* "possible speech contamination in room-noise capture" */
  AF_NOISE_REASON_METADATA = 1u << 12,            /* bits 12 .. 17: AF_NOISE_MISMATCH_* << 12 */
  AF_NOISE_REASON_STALE = 1u << 18,               /* "room-noise reference is stale" */
  AF_NOISE_REASON_MAY_BE_STALE = 1u << 19,        /* "room-noise reference may be stale" */
  AF_NOISE_REASON_MISMATCH = 1u << 20,            /* "room noise does not match conditions during the voice capture" */
  AF_NOISE_REASON_PARTIAL_MATCH = 1u << 21,       /* "room-noise reference only partly matches the voice capture" */
  AF_NOISE_REASON_LEVEL_CHANGED = 1u << 22,       /* "room-noise level changed substantially before the voice capture" */
  AF_NOISE_REASON_MUCH_LOUDER = 1u << 23          /* "room-noise reference is much louder than in-capture quiet frames" */
};
/* the checks of _metadata_mismatches, :223-244, in the order of their reason texts */
enum {
  AF_NOISE_MISMATCH_INPUT_DEVICE = 1u << 0, AF_NOISE_MISMATCH_CHANNEL_MODE = 1u << 1, AF_NOISE_MISMATCH_CHANNEL_COUNT = 1u << 2,
  AF_NOISE_MISMATCH_NOISE_RATE = 1u << 3, AF_NOISE_MISMATCH_VOICE_RATE = 1u << 4, AF_NOISE_MISMATCH_RATE_CHANGED = 1u << 5
};
/* one stream's verdict and the scalars of `metrics`, :511-532; a value the reference leaves None is NaN */
typedef struct af_noise_reference_row {
  int32_t status;          /* AF_NOISE_STATUS_* */
  int32_t conservative;    /* :537 */
  uint32_t reasons;        /* AF_NOISE_REASON_* */
  uint32_t guidance;       /* bit i: the i-th distinct guidance text of :315-470 in source order */
  double quality_score;
  double duration_s, finite_fraction, noise_rms_db, conservative_noise_rms_db, noise_peak_db, crest_factor_db;
  double clipped_fraction, zero_fraction, rms_spread_db, octave_stability_db, spectral_flux_db;
  double vad_contamination_ratio, vad_contamination_p90, capture_age_s, in_capture_level_delta_db, spectral_shape_distance_db;
  double noise_sum_squares, noise_peak;                 /* what the sample-statistics kernel left */
  int64_t finite_samples, clipped_samples, zero_samples;
  int32_t in_capture_noise_frame_count;
  int32_t noise_frames, speech_frames;  /* analysis frames of the two captures (0 below one frame) */
  int32_t n_bands;                      /* octave bands that hold a bin */
  int32_t has_in_capture_spectrum;
  int32_t reserved;
} af_noise_reference_row;
/* Where a call writes; every pointer is host memory and may be null.  bins = af_noise_reference_bins(h, n_noise), F and Fv the
 * frames of the noise and the voice capture, K = frame / 2 + 1.  Spectra are dB. */
typedef struct af_noise_reference_outputs {
  af_noise_reference_row *rows;      /* [n_streams] */
  double *explicit_spectrum_db;      /* [n_streams][bins] the median over the noise frames, :179 (-120 below one frame, :340) */
  double *conservative_spectrum_db;  /* [n_streams][bins] :424, :453 */
  double *in_capture_spectrum_db;    /* [n_streams][bins] :274 on the noise grid (:431-437); a NaN row where it is None */
  double *frame_rms_db;              /* [n_streams][F] :129 */
  double *band_levels_db;            /* [n_streams][F][7] :145, the first n_bands of a row; NaN behind them */
  /* what the kernels left, for tests: */
  double *noise_chunk_sums;          /* [n_streams][F + 1][2] sums of x and x^2 over hop-sized chunks */
  double *noise_frame_power;         /* [n_streams][F] :128 */
  double *speech_frame_power;        /* [n_streams][Fv] */
  double *noise_psd;                 /* [n_streams][F][K] :133-134 */
  double *band_power;                /* [n_streams][F][7] :144 */
  double *explicit_middles;          /* [n_streams][2][K] lower and upper middle of the PSD over the noise frames */
  double *in_capture_middles;        /* [n_streams][2][K] the same over the quiet voice frames; NaN where none were selected */
} af_noise_reference_outputs;
int af_noise_reference_create(uint32_t sample_rate, int32_t device, af_noise_reference **out);
void af_noise_reference_destroy(af_noise_reference *h);
int32_t af_noise_reference_frame_size(const af_noise_reference *h);                /* VALUE */
int32_t af_noise_reference_bins(const af_noise_reference *h, int64_t n_noise);     /* VALUE: frame / 2 + 1; below one frame
                                                                                      max(2, n_noise) / 2 + 1, the grid of :339 */
int64_t af_noise_reference_frames(const af_noise_reference *h, int64_t n_samples); /* VALUE: 0 below one frame */
/* noise: [n_streams][noise_stride] captures of n_noise >= 0 samples.  speech: null, or [n_streams][speech_stride] voice captures
 * of n_speech samples.  noise_vad / speech_vad: null, or [n_streams][n] speech posteriors spread evenly over the capture
 * (_interpolate_vad, :188-205).  capture_age_s: null, or per stream the voice capture's time minus the noise capture's (NaN:
 * unknown; negative counts as 0, :248).  metadata_mismatch: null, or per stream AF_NOISE_MISMATCH_* bits.  _host takes host
 * audio, _device device audio (on the null stream); the other arrays are host memory.  Both return after the outputs are written. */
int af_noise_reference_analyze_host(af_noise_reference *h, const float *noise, int64_t n_noise, int32_t n_streams, int64_t noise_stride,
                                    const float *speech, int64_t n_speech, int64_t speech_stride, const double *noise_vad,
                                    int64_t n_noise_vad, const double *speech_vad, int64_t n_speech_vad, const double *capture_age_s,
                                    const uint32_t *metadata_mismatch, const af_noise_reference_outputs *out);
int af_noise_reference_analyze_device(af_noise_reference *h, const float *d_noise, int64_t n_noise, int32_t n_streams, int64_t noise_stride,
                                      const float *d_speech, int64_t n_speech, int64_t speech_stride, const double *noise_vad,
                                      int64_t n_noise_vad, const double *speech_vad, int64_t n_speech_vad, const double *capture_age_s,
                                      const uint32_t *metadata_mismatch, const af_noise_reference_outputs *out);
/* GPU time of the kernels of the last call: ms[0 .. 4) = sample statistics and chunk sums, frame powers, frame spectra with
 * the band sums, column medians (events around them; copies and host decisions are not in it).  capacity: at least 4. */
int af_noise_reference_last_kernel_ms(af_noise_reference *h, double *ms, int32_t capacity);

/* ---- speech features: python/mic_eq/analysis/voice_setup.py:161-458 ---------------------------------------------
 * _vad_masked_speech_features for a batch of voice captures: frame levels and the VAD-fused active-speech mask (:178-205),
 * momentary and short-term loudness of the active speech (:127-158, :214-261), four robust band levels (:263-289) and the
 * per-frame sibilance evidence with the frame model of deesser_fusion.py:60-78 (:291-430).  Frames are 1920 samples at hop 960.
 * 48000 Hz only: the reference K-weights at 48 kHz behind scipy's resample_poly (:130-132), which af_device_rate_features_*
 * below restates, so any other rate is AF_ERR_UNSUPPORTED at create here.  A capture below one frame is AF_ERR_INVALID_ARGUMENT (the reference raises:
 * its window and frame shapes disagree, :173, :281).  A non-finite sample in a stream's speech capture, or in a whole analysis
 * frame of its noise capture (what the reference reads of it: samples behind the last whole frame are not examined), sets that
 * stream's `non_finite`; none of its other fields is defined then, and the other streams are not affected. */
typedef struct af_speech_features af_speech_features;
/* one stream: every scalar of the dict at :432-458 and of its deesser_frame_evidence, :291-302 / :410-430 */
typedef struct af_speech_features_row {
  int32_t non_finite;
  int32_t frames;                   /* len(frame_db) */
  int32_t active_frames;            /* count of active_frame_mask */
  int32_t spectral_frames;          /* len(frame_indices): active | energy_active, :269 */
  int32_t noise_frames;             /* analysis frames of the noise capture (0: the percentile-10 fallback of :317 holds) */
  int32_t vad_probability_used;
  int32_t short_term_window_count, loudness_window_count;
  int32_t evidence_available;       /* deesser_frame_evidence["available"] */
  int32_t reserved;
  double active_duration_s, active_ratio, vad_active_frame_ratio;
  double short_term_lufs, momentary_lufs, active_loudness_spread_db, loudness_range_db;
  double band_low_db, band_body_db, band_presence_db, band_sibilance_db; /* band_energy_db */
  double sibilance_excess_db;
  double confidence, frame_probability_p90, frame_probability_top_mean, temporal_score, absolute_hf_strength_p90;
  double noise_reliability_p90, excess_p90_db, temporal_contrast_db, candidate_frame_ratio, candidate_snr_db, peak_hz;
  double adaptive_floor_db;         /* :180 */
} af_speech_features_row;
/* Where a call writes; every pointer is host memory and may be null.  F = af_speech_features_frames(n), C =
 * af_speech_features_chunks(n), Fn the same of the noise capture, S = af_speech_features_sibilance_bins(h).  Per-frame rows of
 * the spectrally active frames fill the first spectral_frames entries of a stream's F; the rest is left as it was. */
typedef struct af_speech_features_outputs {
  af_speech_features_row *rows;   /* [n_streams] */
  double *frame_db;               /* [n_streams][F] :179 */
  uint8_t *active_frame_mask;     /* [n_streams][F] :189-205 */
  int32_t *frame_indices;         /* [n_streams][F] :270 */
  double *frame_probabilities;    /* [n_streams][F] :387 */
  double *frame_feature_rows;     /* [n_streams][F][6] :373-386 */
  /* what the kernels left, for tests: */
  double *frame_power;            /* [n_streams][F] :178 */
  double *chunk_energy;           /* [n_streams][C] sums of the squared K-weighted samples over hop-sized chunks */
  double *band_sums;              /* [n_streams][F][8] 80-250 | 250-2000 | 2000-5000 | 5000-10000 | 250-4500 | 5000-9500 Hz | max | 0 */
  double *sibilance_middles;      /* [n_streams][F][2] lower and upper middle of a frame's 5000-9500 Hz bins */
  int32_t *sibilance_argmax;      /* [n_streams][F] :352 */
  double *sibilance_rows;         /* [n_streams][F][S] :347 */
  double *noise_band_sums;        /* [n_streams][Fn] :337 before its logarithm */
  double *weighted_sums;          /* [n_streams][S] :393-397 before the division by the weights' sum */
  int32_t *weighted_argmax;       /* [n_streams] :400 */
} af_speech_features_outputs;
int af_speech_features_create(uint32_t sample_rate, int32_t max_streams, int64_t max_speech_samples, int64_t max_noise_samples,
                              int32_t device, af_speech_features **out);
void af_speech_features_destroy(af_speech_features *h);
int64_t af_speech_features_frames(int64_t n_samples);             /* VALUE: 0 below one frame */
int64_t af_speech_features_chunks(int64_t n_samples);             /* VALUE: hop-sized chunks, the partial tail included */
int32_t af_speech_features_sibilance_bins(const af_speech_features *h); /* VALUE: bins of 5000-9500 Hz (181) */
/* deesser_fusion.py:30-41, FRAME_INTERCEPT and FRAME_COEFFICIENTS (the defaults); non-finite values are refused */
int af_speech_features_set_frame_model(af_speech_features *h, double intercept, const double coefficients[6]);
int af_speech_features_get_frame_model(const af_speech_features *h, double *intercept, double coefficients[6]);
/* speech: [n_streams][speech_stride] captures of n_speech >= 1920 samples.  noise_rms_db: [n_streams].  vad_probabilities:
 * null, or [n_streams][n_vad] posteriors of 1536 samples each (_interpolate_vad_probabilities, spectrum.py:172-197).  noise:
 * null, or [n_streams][noise_stride] captures of n_noise samples.  _host takes host audio, _device device audio (on the null
 * stream); the other arrays are host memory.  Both return after the outputs are written. */
int af_speech_features_analyze_host(af_speech_features *h, const float *speech, int64_t n_speech, int32_t n_streams, int64_t speech_stride,
                                    const double *noise_rms_db, const double *vad_probabilities, int64_t n_vad, const float *noise,
                                    int64_t n_noise, int64_t noise_stride, const af_speech_features_outputs *out);
int af_speech_features_analyze_device(af_speech_features *h, const float *d_speech, int64_t n_speech, int32_t n_streams,
                                      int64_t speech_stride, const double *noise_rms_db, const double *vad_probabilities, int64_t n_vad,
                                      const float *d_noise, int64_t n_noise, int64_t noise_stride, const af_speech_features_outputs *out);
/* GPU time of the kernels of the last call: ms[0 .. 5) = frame powers, K-weighting, frame spectra, medians over frames,
 * weighted peak (events around them; copies and host decisions are not in it).  capacity: at least 5. */
int af_speech_features_last_kernel_ms(af_speech_features *h, double *ms, int32_t capacity);

/* ---- speech features at device rates ------------------------------------------------------------------------------
 * The same measurement for captures at 16000, 22050, 24000, 32000, 44100, 48000, 88200 or 96000 Hz; any other rate is
 * AF_ERR_UNSUPPORTED at create, with the rate and the rule it breaks.  Frames are int(0.04 fs) samples at hop int(0.02 fs), the
 * posteriors cover ceil(fs 512 / 16000) samples each, the sibilance bands end at min(., 0.45 fs).  The loudness K-weights at
 * 48 kHz: signal and sample mask go through scipy.signal.resample_poly(x, 48000 / g, fs / g) (voice_setup.py:127-140, :214-230),
 * restated on the device -- the same polyphase sum in the same order, on a filter designed here that agrees with scipy's to a
 * few ulp of its peak.  Rows, outputs and arguments are af_speech_features_*'s, with F = frames(n), C = chunks(n) = chunks of 960
 * samples of the resampled_length(n) = ceil(n 48000 / fs) samples at 48 kHz.  At 48000 Hz nothing is resampled and every
 * result has af_speech_features_*'s bits. */
typedef struct af_device_rate_features af_device_rate_features;
int af_device_rate_features_create(uint32_t sample_rate, int32_t max_streams, int64_t max_speech_samples, int64_t max_noise_samples,
                                   int32_t device, af_device_rate_features **out);
void af_device_rate_features_destroy(af_device_rate_features *h);
int64_t af_device_rate_features_frames(const af_device_rate_features *h, int64_t n_samples);           /* VALUE: 0 below one frame */
int64_t af_device_rate_features_chunks(const af_device_rate_features *h, int64_t n_samples);           /* VALUE: 48 kHz chunks of 960 */
int64_t af_device_rate_features_resampled_length(const af_device_rate_features *h, int64_t n_samples); /* VALUE */
int32_t af_device_rate_features_sibilance_bins(const af_device_rate_features *h); /* VALUE: 181; 89 at 16 kHz (5000-7200 Hz) */
int af_device_rate_features_set_frame_model(af_device_rate_features *h, double intercept, const double coefficients[6]);
int af_device_rate_features_get_frame_model(const af_device_rate_features *h, double *intercept, double coefficients[6]);
/* The resampled captures pass through scratch a segment of whole 48 kHz chunks of every stream at a time: 9 bytes a sample, at
 * most `bytes` of it (256 MB by default; at least one chunk of every stream).  Results do not depend on it. */
int af_device_rate_features_set_scratch_bytes(af_device_rate_features *h, int64_t bytes);
int af_device_rate_features_analyze_host(af_device_rate_features *h, const float *speech, int64_t n_speech, int32_t n_streams,
                                         int64_t speech_stride, const double *noise_rms_db, const double *vad_probabilities, int64_t n_vad,
                                         const float *noise, int64_t n_noise, int64_t noise_stride, const af_speech_features_outputs *out);
int af_device_rate_features_analyze_device(af_device_rate_features *h, const float *d_speech, int64_t n_speech, int32_t n_streams,
                                           int64_t speech_stride, const double *noise_rms_db, const double *vad_probabilities,
                                           int64_t n_vad, const float *d_noise, int64_t n_noise, int64_t noise_stride,
                                           const af_speech_features_outputs *out);
/* ms[0 .. 6) = frame powers, K-weighting, frame spectra, medians over frames, weighted peak, resampling.  capacity: at least 6. */
int af_device_rate_features_last_kernel_ms(af_device_rate_features *h, double *ms, int32_t capacity);
/* For tests: the resampling stage alone.  active_frames: [n_streams][F] frame flags (host); signal [n_streams][n48] and mask
 * [n_streams][n48] (1 where the resampled sample mask is >= 0.5) with n48 = resampled_length(n_speech); counts [n_streams][C]
 * the set bytes per chunk.  Not for a 48000 Hz handle. */
int af_device_rate_features_debug_resample_host(af_device_rate_features *h, const float *speech, int64_t n_speech, int32_t n_streams,
                                                int64_t speech_stride, const uint8_t *active_frames, double *signal, uint8_t *mask,
                                                int32_t *counts);

/* ---- voice-chain recommendation: python/mic_eq/analysis/voice_setup.py:1143-1223, 468-696 ------------------------------
 * The rules that turn one capture pair's measurements into gate, de-esser and compressor settings: the level percentiles of
 * the active frames (:1143-1153), snr_confidence and capture_confidence with its five caps (:1169-1190),
 * _recommend_gate_settings (:468-502), _recommend_deesser_settings with predict_clip_probability (:505-624,
 * deesser_fusion.py:81-87) and _recommend_compressor_settings (:627-696, :1220-1222).  Host only, f64, no HIP call.  What the
 * other analyses measured comes in as arguments: the speech features, the smoothed median spectrum with residual_confidence,
 * snr_db and used_single_spectrum_fallback of the voice spectrum, and quality_score, status and conservative_noise_rms_db of
 * the noise reference. */
enum { AF_DYNAMICS_GENTLE = 0, AF_DYNAMICS_BALANCED = 1, AF_DYNAMICS_DENSE = 2, AF_DYNAMICS_CUSTOM = 3 };
typedef struct af_voice_setup_inputs {
  const af_speech_features_row *features;  /* of this stream; non_finite must be 0 */
  const double *frame_db;                  /* [features->frames] */
  const uint8_t *active_frame_mask;        /* [features->frames] */
  const double *freqs, *spectrum_db;       /* [bins] the smoothed median spectrum on its grid */
  int32_t bins;
  int32_t used_single_spectrum_fallback;
  double residual_confidence, snr_db;      /* of the voice spectrum */
  double noise_quality_score, conservative_noise_rms_db;
  int32_t noise_status;                    /* AF_NOISE_STATUS_* */
  int32_t vad_available;
  double target_lufs;                      /* TARGET_LUFS_BY_CURVE[target_preset], -18 for an unknown preset (:655) */
  int32_t dynamics_intensity;              /* AF_DYNAMICS_*; anything else counts as balanced (:653) */
  int32_t reserved;
  double custom_target_p95_db, custom_peak_cap_db;
  double enable_probability_threshold;     /* ENABLE_PROBABILITY_THRESHOLD, deesser_fusion.py:57 */
} af_voice_setup_inputs;
typedef struct af_voice_setup_recommendation {
  double speech_floor_db, speech_body_db, speech_frame_peak_db, speech_snr_db, snr_confidence, capture_confidence;
  /* gate, :491-502 (enabled, attack_ms 5 and release_ms 120 are constants) */
  double gate_threshold_db, gate_vad_threshold, gate_vad_hold_time_ms, gate_vad_pre_gain, gate_margin_db;
  int32_t gate_mode, gate_auto_threshold_enabled;
  /* de-esser, :584-623 (auto_enabled, threshold_db -28, attack_ms 2 and release_ms 80 are constants) */
  int32_t deesser_enabled, deesser_frame_evidence_available, deesser_invalid_evidence, reserved;
  double deesser_auto_amount, deesser_low_cut_hz, deesser_high_cut_hz, deesser_ratio, deesser_max_reduction_db;
  double deesser_sibilance_excess_db, deesser_peak_hz, deesser_frame_evidence_confidence, deesser_detection_probability;
  double deesser_clip_features[6];
  /* compressor, :670-695 */
  int32_t compressor_auto_makeup_enabled, compressor_profile; /* AF_DYNAMICS_* actually used */
  double compressor_threshold_db, compressor_ratio, compressor_attack_ms, compressor_release_ms, compressor_makeup_gain_db;
  double compressor_base_release_ms, compressor_target_lufs, compressor_target_p95_db, compressor_target_median_db;
  double compressor_peak_cap_db, compressor_noise_reference_reliability;
} af_voice_setup_recommendation;
/* the defaults of analyze_voice_setup's arguments: broadcast, balanced, 3.5 / 8.0, VAD available, the published threshold */
void af_voice_setup_default_inputs(af_voice_setup_inputs *in);
int af_voice_setup_recommend(const af_voice_setup_inputs *in, af_voice_setup_recommendation *out);

/* ---- compressor candidate sweep: the simulations behind python/mic_eq/analysis/voice_setup.py:699-1079 --------------------
 * _calibrate_compressor_threshold pushes one capture through simulate_auto_eq_chain (python_api.rs:378-714) once per candidate
 * (threshold, ratio, attack, release).  Every candidate of a capture shares the capture's de-esser and EQ output, so here that
 * output (the COMPRESSOR INPUT, an engine run with compressor and limiter disabled) is loaded once with its per-block input
 * rows, and a LANE = one (capture, candidate) pair runs compressor -> limiter -> true-peak limiter from zero state with its own
 * compressor parameters.  The lane's per-block rows equal those of an engine whose uniform preset is that candidate, bit for
 * bit; its af_chain_simulation holds the numeric keys of the reference's result dict (python_api.rs:649-712).
 * The compressor of a lane is Compressor::new plus the setters of python_api.rs:446-470 in that order: threshold, ratio, attack
 * and release from the candidate, makeup gain, adaptive release, base release and the side-chain high-pass from the capture's
 * af_compressor_base; auto-makeup is off (the search simulates with it forced off, voice_setup.py:798-801). */
typedef struct af_compressor_search af_compressor_search;
typedef struct af_compressor_candidate {
  int32_t capture;
  int32_t reserved;
  double threshold_db, ratio, attack_ms, release_ms;
} af_compressor_candidate;
typedef struct af_compressor_base { /* python_api.rs:454-470 */
  double makeup_gain_db, base_release_ms;
  int32_t adaptive_release, sidechain_highpass_enabled;
} af_compressor_base;
typedef struct af_chain_simulation { /* python_api.rs:649-712, the numeric keys */
  float input_sample_peak_db, input_rms_db, output_sample_peak_db, pre_limiter_true_peak_db;
  float output_true_peak_db, output_rms_db, limiter_effective_ceiling_db, sample_headroom_db;
  float pre_limiter_true_peak_headroom_db, true_peak_headroom_db, limiter_gain_reduction_db;
  float true_peak_limiter_gain_reduction_db;
  uint64_t true_peak_limited_events;
  float compressor_gain_reduction_db, deesser_gain_reduction_db;
  float compressor_gain_reduction_median_db, compressor_gain_reduction_p95_db;
  float compressor_gain_reduction_active_ratio, active_output_gain_db, silence_output_gain_db;
  float silence_level_delta_db, compressor_pumping_score_db;
  int32_t non_finite_output;
  float deesser_gain_reduction_median_db, deesser_gain_reduction_p95_db, analysis_block_ms;
  float active_analysis_threshold_db;
  uint64_t active_analysis_block_count, processed_samples;
  /* the linear maxima and the f32 RMS the dB values above are taken from */
  float output_sample_peak, pre_limiter_true_peak, output_true_peak, output_rms;
} af_chain_simulation;
/* Host work only.  The limiter starts as the search's fixed one (voice_setup.py:748-753): ceiling -1.5 dB, release 80 ms,
 * careful output, lookahead 2 ms.  AF_ERR_INVALID_ARGUMENT for a non-finite or non-positive sample rate. */
int af_compressor_search_create(double sample_rate, int32_t device, af_compressor_search **out);
void af_compressor_search_destroy(af_compressor_search *h);
/* python_api.rs:472-487 with control.rs:904-910: the effective ceiling is min(ceiling_db, -1.5) under careful output. */
int af_compressor_search_set_limiter(af_compressor_search *h, double ceiling_db, double release_ms, double lookahead_ms,
                                     int32_t careful_output);
/* The captures: audio [n_captures][stride] (host or device memory) and the engine's rows of the run that produced it,
 * [blocks][n_captures] (host), of which input_sample_peak, input_square_sum and deesser_gain_reduction_db are read.  Blocks are
 * round(0.020 fs) samples, the last one may be partial.  AF_ERR_UNSUPPORTED above 2048 blocks per capture (the fold's LDS).
 * _load_host refuses non-finite samples (AF_ERR_NON_FINITE); _load_device does not look at the audio: the caller guarantees
 * finite samples (an engine's output is) and keeps the memory alive and unchanged while it is loaded.  A non-finite sample
 * cannot fault: the limiter stages zero it, as in the engine. */
int af_compressor_search_load_host(af_compressor_search *h, const float *audio, int64_t n_samples, int32_t n_captures, int64_t stride,
                                   const af_block_stats *input_rows);
int af_compressor_search_load_device(af_compressor_search *h, const float *d_audio, int64_t n_samples, int32_t n_captures,
                                     int64_t stride, const af_block_stats *input_rows);
/* n_lanes candidates in any order and mix of captures; bases: [n_captures]; out: [n_lanes].  keep_audio != 0 also stores every
 * lane's output audio (a test switch: n_lanes x n_samples floats of device memory). */
int af_compressor_search_sweep(af_compressor_search *h, const af_compressor_candidate *lanes, int32_t n_lanes,
                               const af_compressor_base *bases, int32_t keep_audio, af_chain_simulation *out);
/* The last sweep: its rows as [blocks][n_lanes] af_block_stats (the capture's input fields merged in; capacity in rows), its
 * audio as [n_lanes][stride] (AF_ERR_STATE when it was not kept), its two kernel times. */
int64_t af_compressor_search_blocks(const af_compressor_search *h); /* VALUE: control blocks per capture of the loaded batch */
/* What the host derived per capture at load (python_api.rs:578-617): in_db [n_captures][blocks], mask [n_captures][blocks]
 * (bit 0: active, bit 1: audible), active_threshold_db [n_captures]; null pointers are skipped. */
int af_compressor_search_read_masks(const af_compressor_search *h, float *in_db, uint8_t *mask, float *active_threshold_db);
int af_compressor_search_read_rows(af_compressor_search *h, af_block_stats *rows, int64_t capacity);
int af_compressor_search_read_audio(af_compressor_search *h, float *audio, int64_t stride);
int af_compressor_search_last_kernel_ms(af_compressor_search *h, double *sweep_ms, double *fold_ms);

/* _calibrate_compressor_threshold, voice_setup.py:742-1079, for every loaded capture: the incumbent clamped to the bounds
 * (:770-776), phase 1 = incumbent, 33 thresholds and 16 Halton points (:916-926), the objective of :824-914, two refinement
 * seeds with +- steps on the four controls (:937-966), the threshold-only / expanded choice (:968-995) and the winner's
 * verification run (:997-1023): three sweeps per batch (at most 50 and 16 lanes per capture, then one).  The limiter should be
 * the search's fixed one (the default of af_compressor_search_create).  With auto_makeup_enabled the simulations run with
 * auto-makeup off and makeup 0 (:798-801).  Without a feasible candidate backend_available is 0, the four controls are the
 * settings' own and iterations counts the evaluations (:932-935). */
typedef struct af_compressor_search_settings {
  double threshold_db, ratio, attack_ms, release_ms; /* the compressor settings to calibrate */
  double makeup_gain_db, base_release_ms;
  int32_t adaptive_release, sidechain_highpass_enabled, auto_makeup_enabled, reserved;
  double target_lufs, measured_short_term_lufs;      /* -18 each when the settings have none (:833-838) */
  double target_p95_db, target_median_db, peak_cap_db;
} af_compressor_search_settings;
typedef struct af_compressor_search_result {
  int32_t backend_available, expanded_search_selected, peak_cap_passed, iterations, candidate_count;
  int32_t evaluated_count;      /* candidates simulated and scored, without the verification */
  int32_t winner;               /* its index in `evaluated`, -1 without a feasible candidate */
  int32_t verification_equals_evaluation; /* the verification's record equals the winner's first one, byte for byte */
  double threshold_db, ratio, attack_ms, release_ms; /* calibrated */
  double measured_median_gain_reduction_db, measured_p95_gain_reduction_db, measured_peak_gain_reduction_db, active_reduction_ratio;
  double total_objective, incumbent_objective, threshold_only_objective, expanded_candidate_objective;
  double active_output_gain_db, silence_output_gain_db, compressor_pumping_score_db, output_true_peak_db;
  double pre_limiter_true_peak_headroom_db;
  double evaluated[67][4];      /* in evaluation order: threshold_db, ratio, attack_ms, release_ms as simulated */
  double scores[67];            /* +inf: hard-rejected */
} af_compressor_search_result;
int af_compressor_search_run(af_compressor_search *h, const af_compressor_search_settings *settings, af_compressor_search_result *out);
/* kernel ms of the last run's three sweeps: phase 1 sweep, fold; phase 2 sweep, fold; verification sweep, fold */
int af_compressor_search_last_run_ms(const af_compressor_search *h, double ms[6]);

/* ---- per-lane EQ: the EQ half of the renders behind python/mic_eq/analysis/auto_eq_parts/headroom.py:292-354 -------------
 * apply_headroom_validation pushes one capture through simulate_auto_eq_chain (python_api.rs:378-714) once per gain scale: the
 * same audio through ten-band EQs that differ only in their gains.  Here a LANE = one (capture, band set) pair runs the EQ of
 * that chain over its capture's row, from zero state, with its own coefficients: ParametricEQ::new(sample_rate)
 * (eq.rs:357-368), then set_band_frequency, set_band_gain, set_band_q per band in that order (python_api.rs:408-412, the legacy
 * (frequency_hz, gain_db, q) triples), then ParametricEQ::process_block_inplace (eq.rs:371-379) with the coefficient crossfade
 * the setters scheduled (biquad.rs:249-327).  Non-finite input samples are zeroed first (python_api.rs:517-520).  A lane's output
 * equals the compressor input of an engine configured with the lane's bands and nothing but the EQ enabled, bit for bit.
 * The output stays on the device as [n_lanes][stride] float32 and is what af_compressor_search_load_device takes. */
typedef struct af_lane_eq af_lane_eq;
/* Host work only.  AF_ERR_INVALID_ARGUMENT for a non-finite or non-positive sample rate and for device < 0. */
int af_lane_eq_create(double sample_rate, int32_t device, af_lane_eq **out);
void af_lane_eq_destroy(af_lane_eq *h);
/* audio: [n_captures][stride] float32 (host memory / device memory); lane_capture: HOST memory, [n_lanes], each in
 * 0..n_captures-1, in any order and mix; bands: HOST memory, [n_lanes][10][3] doubles (frequency_hz, gain_db, q).
 * Arguments are checked before any GPU work: AF_ERR_INVALID_ARGUMENT for a null pointer, n_samples <= 0, n_captures <= 0,
 * n_lanes <= 0, stride < n_samples, a lane_capture out of range, a band value that is not finite.  _run_device does not look at
 * the audio and keeps no reference to it after the kernel has run; both calls return when the kernel has been enqueued on the
 * device's null stream (the readers below wait for it). */
int af_lane_eq_run_host(af_lane_eq *h, const float *audio, int64_t n_samples, int32_t n_captures, int64_t stride,
                        const int32_t *lane_capture, int32_t n_lanes, const double *bands);
int af_lane_eq_run_device(af_lane_eq *h, const float *d_audio, int64_t n_samples, int32_t n_captures, int64_t stride,
                          const int32_t *lane_capture, int32_t n_lanes, const double *bands);
/* The last run's output on the device: [n_lanes][*stride] float32, *stride >= n_samples (rows start 256 B aligned); valid until
 * the next run on the handle or its destruction.  AF_ERR_STATE before the first run. */
int af_lane_eq_output(af_lane_eq *h, float **d_out, int64_t *stride);
/* The last run's output to host memory as [n_lanes][stride], n_samples per row. */
int af_lane_eq_read_output(af_lane_eq *h, float *out, int64_t stride);
int af_lane_eq_last_kernel_ms(af_lane_eq *h, double *ms);

/* ---- streaming lane chain: one processor per stream, each under its own settings ------------------------------------------
 * The reference configures one processor per caller (python/mic_eq/config_parts/settings.py:543-593).  An af_engine preset is a
 * 64-stream group; here ONE STREAM IS ONE LANE and carries its own settings and its own state from call to call.  Every stream
 * runs the dynamics chain simulate_auto_eq_chain configures (python_api.rs:400-487) without the de-esser, in
 * OfflineDspBlockProcessor's order (block_processor.rs:106-161): input scrub (python_api.rs:517-520) -> ParametricEQ (ten legacy
 * bands, with the coefficient crossfade the setters schedule) -> Compressor (auto-makeup off) -> Limiter -> TruePeakLimiter ->
 * block output statistics and TruePeakDetector.  Every call starts a new control block of round(0.020 * sample_rate) samples
 * clamped to 1..8192 (python_api.rs:512-514); the last block of a call may be short.  A stream's output and rows equal, bit for
 * bit, those of a one-stream af_engine configured with the stream's settings and driven with the same calls.
 * Not here (they stay with af_engine): the de-esser, auto-makeup, typed EQ bands, the gate, the suppressor, the front-end
 * filters, device-rate I/O, live retune without a restart, state export and import. */
typedef struct af_lane_chain af_lane_chain;
/* One stream's settings: the keys of simulate_auto_eq_chain's settings dict (python_api.rs:400-487) that this object runs. */
typedef struct af_lane_chain_settings {
  double bands[10][3];                 /* (frequency_hz, gain_db, q): set_band_frequency / _gain / _q, python_api.rs:408-412 */
  double compressor_threshold_db, compressor_ratio, compressor_attack_ms, compressor_release_ms; /* python_api.rs:446-456 */
  double compressor_makeup_gain_db, compressor_base_release_ms;
  double limiter_ceiling_db, limiter_release_ms;  /* effective ceiling min(ceiling, -1.5) under careful output, control.rs:904-910;
                                                     the true-peak limiter's release is limiter_release_ms as an f32 */
  int32_t eq_enabled, compressor_enabled, limiter_enabled;  /* OfflineDspBlockProcessor's stage switches, block_processor.rs:31-60 */
  int32_t compressor_adaptive_release, compressor_sidechain_highpass_enabled, limiter_careful_output_enabled;
} af_lane_chain_settings;
/* simulate_auto_eq_chain's defaults (python_api.rs:400-487) with flat bands at the default frequencies (eq.rs:122-138). */
int af_lane_chain_default_settings(af_lane_chain_settings *out);
/* OfflineDspBlockProcessor::new per stream (block_processor.rs:31-60): host work only.  limiter_lookahead_ms is the object's
 * (Limiter::set_lookahead_ms, limiter.rs:154-184) and sets the height of every stream's delay ring.  AF_ERR_INVALID_ARGUMENT for
 * a null `out`, a sample_rate or limiter_lookahead_ms that is not finite and positive, n_streams <= 0, device < 0.  A stream
 * that is never configured runs OfflineDspBlockProcessor's defaults: flat EQ, compressor off, limiter at -0.5 dB. */
int af_lane_chain_create(double sample_rate, int32_t n_streams, double limiter_lookahead_ms, int32_t device, af_lane_chain **out);
void af_lane_chain_destroy(af_lane_chain *h);
/* The listed streams become fresh processors with settings[i]: OfflineDspBlockProcessor::new plus the setters in
 * python_api.rs:400-487's order, which leaves the EQ's coefficient crossfade pending.  Every other stream continues
 * undisturbed.  Host work only (the streams' columns are uploaded with the next process call).  AF_ERR_INVALID_ARGUMENT, with
 * nothing changed, for a null pointer, n <= 0, a stream index out of range or listed twice, a value that is not finite. */
int af_lane_chain_configure(af_lane_chain *h, const int32_t *streams, int32_t n, const af_lane_chain_settings *settings);
/* OfflineDspBlockProcessor::process_block_inplace (block_processor.rs:106-161) per control block over [n_streams][stride]
 * float32, n_samples per row; out may equal in.  n_samples == 0 is a no-op.  AF_ERR_INVALID_ARGUMENT before any device work
 * for a null pointer, n_samples < 0, stride < n_samples.  _host returns when the output is in `out`; _device enqueues on
 * `hip_stream` (a hipStream_t, NULL = default stream) and keeps no reference to the buffers after the kernel has run; columns
 * waiting from af_lane_chain_configure / _reset go first on the same stream, through pinned staging, without a host wait.  The
 * host waits only when the stream differs from the last call's (for that call) or a buffer of the object has to grow.  The
 * caller's current device is the same after every af_lane_chain_* call as before it. */
int af_lane_chain_process_host(af_lane_chain *h, const float *in, float *out, int64_t n_samples, int64_t stride);
int af_lane_chain_process_device(af_lane_chain *h, const float *d_in, float *d_out, int64_t n_samples, int64_t stride,
                                 void *hip_stream);
/* Control blocks of the last process call, and their rows as [blocks][n_streams] af_block_stats (BlockStats of
 * block_processor.rs:106-161, input fields included; capacity in rows; waits for the call). */
int64_t af_lane_chain_blocks(const af_lane_chain *h);
int af_lane_chain_read_rows(af_lane_chain *h, af_block_stats *rows, int64_t capacity);
/* OfflineDspBlockProcessor::new for EVERY stream with its current settings (as af_lane_chain_configure of all streams). */
int af_lane_chain_reset(af_lane_chain *h);
/* Samples the stream has processed since it was last configured or reset. */
int af_lane_chain_samples_processed(const af_lane_chain *h, int32_t stream, int64_t *out);
int af_lane_chain_last_kernel_ms(af_lane_chain *h, double *ms);

/* ---- second-passage verification, the measurements: python/mic_eq/analysis/voice_setup.py:1446-1679 ---------------------
 * validate_voice_setup_verification renders a second passage and the room tone through the recommended chain and measures both
 * sides.  This object takes what the other analyses leave (the median spectra of the original, the verification and the
 * rendered passage from af_voice_spectrum_*, the rendered side's spectral SNR, and the five signals) and returns, per stream,
 * the numbers the reference's decision reads that no other entry point yields:
 *   _shape_error_db (:1446-1465) of the before and the after side against the adaptive house curve
 *     (auto_eq_parts/target.py:15-104 over TARGET_CURVES / EQ_FREQUENCIES), with the five scalars the adaptive offsets were
 *     derived from (body, presence and sibilance means, tilt in dB/octave, low-mid balance: target.py:24-43);
 *   the repeatability delta (:1562-1575);
 *   the medians of the after side's spectral SNR over low 80-250 | body 250-1000 | presence 1000-4500 | sibilance 4500-10000 Hz
 *     (:1634-1645), lower edge inclusive, upper exclusive, NaN as np.median, a band without bins absent;
 *   per signal the f64 sum of squares in NumPy's pairwise order and _rms_db of it (:102-106), the peak, whether a sample is not
 *     finite, and the clipped tests of :1490 (>= 0.999) and :1677 (>= 1.0).
 * The three spectra share the grid np.fft.rfftfreq(nperseg, 1 / sample_rate), on which the np.interp of :1562-1566 returns the
 * original's own values.  af_setup_verification_decide below turns a row and the simulation's numbers into accept / reduce /
 * rollback / retry.  Sum orders: csrc/af_setup_verification_math.h. */
enum { AF_TARGET_BROADCAST = 0, AF_TARGET_PODCAST = 1, AF_TARGET_STREAMING = 2, AF_TARGET_FLAT = 3, AF_TARGET_PRESET_COUNT = 4 };
enum { /* the signals of one stream, in the order of every [AF_SETUP_SIGNALS] array */
  AF_SETUP_SIGNAL_NOISE = 0, AF_SETUP_SIGNAL_ORIGINAL = 1, AF_SETUP_SIGNAL_VERIFICATION = 2, AF_SETUP_SIGNAL_RENDERED = 3,
  AF_SETUP_SIGNAL_RENDERED_NOISE = 4, AF_SETUP_SIGNALS = 5
};
typedef struct af_setup_verification af_setup_verification;
typedef struct af_setup_verification_audio {
  const float *samples;   /* [n_streams][stride]; NULL: the signal is absent (zero sums and flags, rms_db -120) */
  int64_t stride;         /* >= length */
  int64_t length;         /* samples per stream */
  const int64_t *lengths; /* HOST memory in both entry points, [n_streams], each in 0..length; NULL: `length` for every stream */
} af_setup_verification_audio;
typedef struct af_setup_verification_row {
  int32_t masked_bins;      /* bins in 80..12000 Hz; below 8 both errors are +inf (:1455-1456) */
  int32_t snr_available;    /* 0: no spectral SNR was given, frequency_dependent_snr_db is empty (:1636) */
  int32_t band_present[4];
  int32_t non_finite[5], clipped_0999[5], clipped_1[5];
  int32_t reserved;
  double spectral_target_error_before_db, spectral_target_error_after_db; /* :1552-1561 */
  double shape_delta_db;                                                  /* :1575; NaN without a masked bin */
  double band_snr_db[4];                                                  /* 0 where absent */
  double offsets_before[5], offsets_after[5]; /* body | presence | sibilance means, tilt dB/octave, low-mid balance; 0 below 8 bins */
  double sum_squares[5], peak[5], rms_db[5];
} af_setup_verification_row;
/* Host work only.  AF_ERR_UNSUPPORTED for a rate other than 48000 and for nperseg above 16384 (the kernel's LDS sort holds
 * 4096 masked bins); AF_ERR_INVALID_ARGUMENT for nperseg odd or below 2, max_streams < 1, device < 0. */
int af_setup_verification_create(uint32_t sample_rate, int32_t nperseg, int32_t max_streams, int32_t device, af_setup_verification **out);
void af_setup_verification_destroy(af_setup_verification *v);
/* original_db, before_db, after_db: [n_streams][spectrum_stride] rows of nperseg / 2 + 1 bins; after_snr_db: the same shape
 * with its own stride, or NULL; preset_ids: HOST memory in both entry points, [n_streams] AF_TARGET_* (any other id:
 * AF_ERR_INVALID_ARGUMENT "Unknown target preset", target.py:78-79); audio: AF_SETUP_SIGNALS entries; rows: [n_streams].
 * Arguments are checked before any GPU work.  _device takes device pointers for spectra, SNR, samples and rows, and enqueues
 * on hip_stream; a non-finite sample cannot fault and is reported in non_finite.  The first call on a handle allocates its
 * device buffers and uploads the grid synchronously; later calls only enqueue, and the preset ids and lengths are the caller's
 * again when the call returns.  A handle holds one copy of the presets and the lengths on the device: calls on one handle go to
 * one stream, or are separated by a synchronisation; use one handle per stream otherwise. */
int af_setup_verification_measure_host(af_setup_verification *v, int32_t n_streams, const double *original_db, const double *before_db,
                                       const double *after_db, int64_t spectrum_stride, const double *after_snr_db, int64_t snr_stride,
                                       const int32_t *preset_ids, const af_setup_verification_audio *audio,
                                       af_setup_verification_row *rows);
int af_setup_verification_measure_device(af_setup_verification *v, int32_t n_streams, const double *d_original_db,
                                         const double *d_before_db, const double *d_after_db, int64_t spectrum_stride,
                                         const double *d_after_snr_db, int64_t snr_stride, const int32_t *preset_ids,
                                         const af_setup_verification_audio *audio, af_setup_verification_row *d_rows, void *hip_stream);

/* The rules of validate_voice_setup_verification for one stream, voice_setup.py:1484-1495 and :1590-1679: host work only.
 * The early exits (:1484-1495, :1527-1537) return three keys in the reference: early_exit is 1 and only decision and reason
 * are meaningful.  Otherwise the ladder of :1608-1632 in its order: retry, then rollback, then reduce, then accept.
 * A key the simulation dict or the settings lack is marked by a cleared bit in `present` and takes the reference's default:
 * 120 for the two compressor reductions and the output true peak (:1593-1597), -1.5 for the ceiling (:1598), 0 events (:1599),
 * the measured _rms_db of the rendered / the verification passage for output_rms_db / input_rms_db (:1601-1603), 0 for the
 * de-esser and median reductions (:1624, :1664-1674), 3.5 / 8.0 / 6.0 for target_p95_reduction_db / peak_reduction_cap_db /
 * max_reduction_db (:1591-1592, :1625). */
enum { AF_SETUP_ACCEPT = 0, AF_SETUP_REDUCE = 1, AF_SETUP_ROLLBACK = 2, AF_SETUP_RETRY = 3 };
enum { /* reasons[0] of the reference's result: af_setup_verification_reason_text */
  AF_SETUP_REASON_PASSED = 0,       /* :1632 */
  AF_SETUP_REASON_STRONGER = 1,     /* :1629 */
  AF_SETUP_REASON_WORSENED = 2,     /* :1619 */
  AF_SETUP_REASON_DIFFERS = 3,      /* :1610 */
  AF_SETUP_REASON_TOO_SHORT = 4,    /* :1487 */
  AF_SETUP_REASON_CLIPPED = 5,      /* :1493 */
  AF_SETUP_REASON_NO_RENDERER = 6,  /* :1534 */
  AF_SETUP_REASON_COUNT = 7
};
enum { /* bits of af_setup_verification_evidence.present */
  AF_SETUP_HAS_COMPRESSOR_P95 = 1 << 0, AF_SETUP_HAS_COMPRESSOR_PEAK = 1 << 1, AF_SETUP_HAS_OUTPUT_TRUE_PEAK = 1 << 2,
  AF_SETUP_HAS_CEILING = 1 << 3, AF_SETUP_HAS_LIMITED_EVENTS = 1 << 4, AF_SETUP_HAS_OUTPUT_RMS = 1 << 5,
  AF_SETUP_HAS_INPUT_RMS = 1 << 6, AF_SETUP_HAS_DEESSER_P95 = 1 << 7, AF_SETUP_HAS_COMPRESSOR_MEDIAN = 1 << 8,
  AF_SETUP_HAS_DEESSER_MEDIAN = 1 << 9, AF_SETUP_HAS_TARGET_P95 = 1 << 10, AF_SETUP_HAS_PEAK_CAP = 1 << 11,
  AF_SETUP_HAS_DEESSER_MAX_REDUCTION = 1 << 12
};
typedef struct af_setup_verification_evidence { /* what the rules read beside the measured row */
  uint32_t present;
  int32_t backend_is_rust;          /* simulation_backend == "rust" and both renders returned audio (:1527-1531) */
  int64_t verification_samples;     /* :1484 */
  double sample_rate;
  uint64_t true_peak_limited_events;
  /* the simulation dict of the verification passage (python_api.rs:649-712) */
  double compressor_gain_reduction_p95_db, compressor_gain_reduction_db, output_true_peak_db, limiter_effective_ceiling_db;
  double output_rms_db, input_rms_db, deesser_gain_reduction_p95_db, compressor_gain_reduction_median_db;
  double deesser_gain_reduction_median_db;
  /* compressor_settings and deesser_settings */
  double target_p95_reduction_db, peak_reduction_cap_db, deesser_max_reduction_db;
  /* VoiceSpectrum.snr_db of the two sides (:1605) and active_loudness_spread_db of the two feature runs (:1655-1660) */
  double before_snr_db, after_snr_db, loudness_variation_before_db, loudness_variation_after_db;
} af_setup_verification_evidence;
typedef struct af_setup_verification_result { /* :1647-1679; frequency_dependent_snr_db is the row's band_snr_db */
  int32_t decision, reason, early_exit, clipped;
  uint64_t limiter_activity_events;
  double spectral_target_error_before_db, spectral_target_error_after_db;
  double loudness_variation_before_db, loudness_variation_after_db;
  double noise_floor_change_db, relative_noise_floor_change_db, snr_change_db;
  double compressor_gain_reduction_median_db, compressor_gain_reduction_p95_db, compressor_gain_reduction_peak_db;
  double deesser_gain_reduction_median_db, deesser_gain_reduction_p95_db, output_true_peak_db;
  double level_difference_db, shape_delta_db; /* what the retry test read (:1608) */
} af_setup_verification_result;
int af_setup_verification_decide(const af_setup_verification_row *row, const af_setup_verification_evidence *evidence,
                                 af_setup_verification_result *out);
const char *af_setup_verification_reason_text(int32_t reason); /* VALUE: NULL for an unknown index */

/* The offline validation and the confidences behind apply_recommended, voice_setup.py:1265-1364, for one stream: host work only.
 * The caller simulates the setup passage through the recommended chain (:1297-1312) and hands over what the rules read.
 * uncertainty_reasons (:1332-1356) come back as bits in the reference's order, after the noise reference's own reasons (which
 * the caller holds): af_setup_offline_reason_text. */
enum {
  AF_SETUP_UNCERTAIN_LITTLE_SPEECH = 1 << 0,  /* "too little VAD-active speech", :1335 */
  AF_SETUP_UNCERTAIN_WEAK_SNR = 1 << 1,       /* :1337 */
  AF_SETUP_UNCERTAIN_UNSTABLE = 1 << 2,       /* :1339 */
  AF_SETUP_UNCERTAIN_NOT_PASSED = 1 << 3,     /* :1341 */
  AF_SETUP_UNCERTAIN_ADVISORY = 1 << 4,       /* :1343 */
  AF_SETUP_UNCERTAIN_EQ_ABSTAINED = 1 << 5,   /* :1356 */
  AF_SETUP_UNCERTAIN_COUNT = 6
};
typedef struct af_setup_offline_inputs {
  double capture_confidence, snr_confidence;          /* af_voice_setup_recommendation */
  double speech_dynamic_range_db;                     /* features' loudness_range_db, :1152 */
  double conservative_noise_rms_db, noise_referenced_snr_db, active_duration_s;
  double deesser_frame_evidence_confidence;
  double peak_reduction_cap_db, target_p95_reduction_db; /* compressor diagnostics, :1324-1326 */
  double eq_analysis_confidence;                      /* read when eq_has_analysis_confidence, :1271 */
  int32_t deesser_enabled, noise_status_usable;
  int32_t has_eq_settings, eq_has_analysis_confidence, eq_apply_recommended; /* eq_settings.get("apply_recommended", True) */
  int32_t simulation_available;                       /* 0: simulate_candidate_chain raised (:1329-1330) */
  int32_t backend_is_rust;
  uint32_t present;                                   /* AF_SETUP_HAS_OUTPUT_TRUE_PEAK | _CEILING | _COMPRESSOR_PEAK | _COMPRESSOR_P95 | AF_SETUP_HAS_DEESSER_PEAK */
  double output_true_peak_db, limiter_effective_ceiling_db, compressor_gain_reduction_db, compressor_gain_reduction_p95_db;
  double deesser_gain_reduction_db;
} af_setup_offline_inputs;
enum { AF_SETUP_HAS_DEESSER_PEAK = 1 << 13 };
typedef struct af_setup_offline_result {
  int32_t offline_validation_passed, weak_capture, apply_recommended;
  uint32_t uncertainty_reasons;
  double eq_confidence, gate_confidence, deesser_confidence, compressor_confidence, setup_confidence, recommendation_uncertainty;
} af_setup_offline_result;
int af_setup_offline_validation(const af_setup_offline_inputs *in, af_setup_offline_result *out);
const char *af_setup_offline_reason_text(int32_t bit_index); /* VALUE: NULL for an unknown index */

/* ---- latency calibration: python/mic_eq/analysis/latency_calibration.py -------------------------------------------------
 * analyze_latency (:232-515) for a batch of recordings of one probe at one sample rate.  The probe is a repeated Barker-13
 * burst (generate_probe_signal :45-71, _coded_probe_components :74-115); a recording's route delay is estimated from the
 * normalised cross-correlation of the whole probe (:137-168, here a direct f64 sum per lag), a local search per burst
 * (:359-384) and a GCC-PHAT cross-check (:171-198: one forward real transform of the recording, the whitened product with the
 * burst's transform, one inverse transform, a windowed first-argmax per burst).  The passes run back to back on the device's
 * null stream with no host wait between them: the burst windows depend on the whole-probe peak and are computed on the device.
 * The rules of :424-515 (medians, the 75th percentile of the deviations, the confidence, success, the message) run on the host
 * when the results are read.  Sum orders: csrc/af_latency_math.h.  Recordings are float32; the probe is taken as doubles.
 * One addition over the reference: a recording with a sample that is not finite is not analysed (AF_LATENCY_EXIT_NON_FINITE);
 * the reference has no such check and would return NaNs.
 * The PHAT transform of a stream has n = the next power of two >= recording + burst real points; n above 2^18 (5.4 s at 48 kHz)
 * is refused. */
enum { /* why a stream was not analysed: the reference's early exits in their order (:254, :279, :314, :336), then ours */
  AF_LATENCY_EXIT_NONE = 0, AF_LATENCY_EXIT_ROUTE = 1, AF_LATENCY_EXIT_SHORT = 2, AF_LATENCY_EXIT_WINDOW = 3,
  AF_LATENCY_EXIT_NO_OVERLAP = 4, AF_LATENCY_EXIT_NON_FINITE = 5, AF_LATENCY_EXIT_COUNT = 6
};
enum { /* :487-494 */
  AF_LATENCY_MESSAGE_OK = 0, AF_LATENCY_MESSAGE_DISAGREE = 1, AF_LATENCY_MESSAGE_ECHO = 2, AF_LATENCY_MESSAGE_LOW_CONFIDENCE = 3,
  AF_LATENCY_MESSAGE_COUNT = 4
};
enum { /* the spans of af_latency_last_kernel_ms */
  AF_LATENCY_PASS_CONDITION = 0, AF_LATENCY_PASS_PROBE = 1, AF_LATENCY_PASS_BURSTS = 2, AF_LATENCY_PASS_PHAT = 3, AF_LATENCY_PASSES = 4
};
enum { AF_LATENCY_MAX_OFFSETS = 4, AF_LATENCY_MAX_TRANSFORM = 1 << 18 };
typedef struct af_latency af_latency;
typedef struct af_latency_search { /* the keywords of analyze_latency for one stream; has_*: the keyword is not None */
  double min_search_ms, max_search_ms;
  double expected_playback_start_ms, expected_playback_jitter_ms, expected_latency_min_ms, expected_latency_max_ms;
  int32_t has_playback_start, has_playback_jitter, has_latency_min, has_latency_max;
  int32_t route_supported; /* route_kind is "output_to_input" after strip().lower(), :253-254 */
  int32_t reserved;
} af_latency_search;
typedef struct af_latency_result {
  int32_t success, exit_code, message, repetition_count; /* message is read only when exit_code is AF_LATENCY_EXIT_NONE */
  int64_t peak_sample_offset;
  double measured_round_trip_ms, applied_compensation_ms, confidence, agreement_ms, ambiguity_score, sub_sample_offset,
      route_latency_ms;
} af_latency_result;
/* Host work only: the burst and its offsets (:325-328), the centred probe and burst with their energies (:276, :160), the
 * twiddle table.  AF_ERR_INVALID_ARGUMENT for a sample_rate that is not finite and positive, a null or non-finite probe, a
 * probe_samples below 16, max_streams < 1, max_record_samples < 1, device < 0, and a max_record_samples whose transform
 * (max_record_samples + burst) would exceed AF_LATENCY_MAX_TRANSFORM real points. */
int af_latency_create(double sample_rate, const double *probe, int64_t probe_samples, int32_t max_streams, int64_t max_record_samples,
                      int32_t device, af_latency **out);
void af_latency_destroy(af_latency *h);
/* The burst's layout: *n_offsets <= AF_LATENCY_MAX_OFFSETS starts into offsets, the burst's length, the local radius (:351). */
int af_latency_layout(af_latency *h, int32_t *n_offsets, int32_t *offsets, int32_t *burst_samples, int32_t *local_radius);
/* recorded: [n_streams][stride] float32 (host memory / device memory), stream s holding lengths[s] samples (NULL: n_samples
 * each; HOST memory either way); search: HOST memory, one per stream.  Arguments are checked before any GPU work:
 * AF_ERR_INVALID_ARGUMENT for a null pointer, n_streams outside 1..max_streams, n_samples outside 1..max_record_samples,
 * stride < n_samples, a length outside 0..n_samples, a search value that is not finite.  Both return when the kernels have been
 * enqueued; _analyze_device keeps no reference to the recordings after they have run. */
int af_latency_analyze_host(af_latency *h, const float *recorded, int64_t n_samples, int64_t stride, int32_t n_streams,
                            const int64_t *lengths, const af_latency_search *search);
int af_latency_analyze_device(af_latency *h, const float *d_recorded, int64_t n_samples, int64_t stride, int32_t n_streams,
                              const int64_t *lengths, const af_latency_search *search);
/* Waits for the last analysis and folds each stream's record into its result.  AF_ERR_STATE before the first analysis. */
int af_latency_read_results(af_latency *h, af_latency_result *out, int32_t n_streams);
/* Diagnostics of one stream of the last analysis.  which = 0: the whole-probe search; 1 + k: the window of burst k.
 * *lag_lo and *count: the lags scored; scores, window_energy: [*count] (NULL: not wanted); phat: the PHAT correlation at the
 * lags *phat_lo .. *phat_lo + *phat_count - 1 of burst k's window (which >= 1 only).  capacity: what each array holds;
 * AF_ERR_INVALID_ARGUMENT when it is too small (the counts are still returned). */
int af_latency_read_scores(af_latency *h, int32_t stream, int32_t which, int32_t *lag_lo, int32_t *count, double *scores,
                           double *window_energy, int32_t *phat_lo, int32_t *phat_count, double *phat, int64_t capacity);
/* The span of the last analysis and, when pass_ms is not NULL, its AF_LATENCY_PASSES parts. */
int af_latency_last_kernel_ms(af_latency *h, double *ms, double *pass_ms);
const char *af_latency_message_text(int32_t exit_code, int32_t message); /* VALUE: NULL for unknown indices */
/* Test hook: the forward real transform of the PHAT pass alone.  x: HOST memory, n_real float32, n_real a power of two in
 * 2^9..AF_LATENCY_MAX_TRANSFORM; out: HOST memory, n_real / 2 + 1 (re, im) pairs.  Up to 2^14 real points it is the
 * one-workgroup LDS form, above that the four-step form. */
int af_latency_debug_rfft(af_latency *h, const float *x, int64_t n_real, double *out);

/* ---- NoiseSuppressor: rust-core/src/dsp/noise_suppressor.rs:18-194 ----------------------------------------
 * The runtime-selected suppressor interface (`NoiseModel`, trait `NoiseSuppressor`, `new_noise_suppression_engine`) for a
 * batch of streams that advance in lock step: sample counts are per stream, audio is [stream][stride] host memory, the
 * two fixed rings hold 8192 + 480 samples per stream (rnnoise.rs:11).  Model ids as NoiseModel::from_id / id(); the
 * DeepFilterNet variants parse but cannot be created (AF_ERR_UNSUPPORTED: the reference loads them from a runtime
 * library + model archives that are not in its checkout, deepfilter_ffi.rs:9-16), and af_noise_model_available lists
 * what a default build of the reference lists: RNNoise. */
enum { AF_NOISE_MODEL_RNNOISE = 0, AF_NOISE_MODEL_DEEPFILTER_LL = 1, AF_NOISE_MODEL_DEEPFILTER = 2 };
typedef struct af_noise_suppressor af_noise_suppressor;
int af_noise_model_from_id(const char *id, int32_t *model);           /* noise_suppressor.rs:58-67 */
const char *af_noise_model_id(int32_t model);                         /* noise_suppressor.rs:47-55; VALUE */
const char *af_noise_model_display_name(int32_t model);               /* noise_suppressor.rs:36-44; VALUE */
int32_t af_noise_model_available(int32_t *models, int32_t capacity);  /* noise_suppressor.rs:70-84; VALUE: count */
int af_noise_suppressor_create(int32_t model, int32_t n_streams, int32_t device, af_noise_suppressor **out); /* :168-194 */
void af_noise_suppressor_destroy(af_noise_suppressor *s);
/* the engine behind it (weights: af_suppressor_load_weights / af_suppressor_set_synthetic_weights before the first frame) */
af_engine *af_noise_suppressor_engine(af_noise_suppressor *s);
/* VALUE functions: sample counts per stream (negative af_status on a bad argument) */
int64_t af_noise_suppressor_push_samples(af_noise_suppressor *s, const float *samples, int64_t n, int64_t stride);
int af_noise_suppressor_process_frames(af_noise_suppressor *s);
int64_t af_noise_suppressor_available_samples(const af_noise_suppressor *s);
int64_t af_noise_suppressor_pending_input(const af_noise_suppressor *s);
int64_t af_noise_suppressor_pop_samples_into(af_noise_suppressor *s, float *out, int64_t count, int64_t stride);
int64_t af_noise_suppressor_drain_pending_input(af_noise_suppressor *s, float *out, int64_t capacity, int64_t stride);
int af_noise_suppressor_set_strength(af_noise_suppressor *s, float value);   /* clamps to [0, 1] */
float af_noise_suppressor_get_strength(const af_noise_suppressor *s);        /* VALUE */
int af_noise_suppressor_set_enabled(af_noise_suppressor *s, int32_t enabled); /* disabled = bit-exact passthrough */
int32_t af_noise_suppressor_is_enabled(const af_noise_suppressor *s);        /* VALUE */
int af_noise_suppressor_soft_reset(af_noise_suppressor *s);                  /* rings cleared, model state kept */
int af_noise_suppressor_reset(af_noise_suppressor *s);                       /* rnnoise.rs:205-210 */
int32_t af_noise_suppressor_model_type(const af_noise_suppressor *s);        /* VALUE */
int32_t af_noise_suppressor_latency_samples(const af_noise_suppressor *s);   /* VALUE: 480 */
int32_t af_noise_suppressor_backend_available(const af_noise_suppressor *s); /* VALUE */
int32_t af_noise_suppressor_backend_failed(const af_noise_suppressor *s);    /* VALUE */
const char *af_noise_suppressor_backend_error(const af_noise_suppressor *s); /* VALUE: NULL = none */

/* ---- stateless helpers ----------------------------------------------------------- */
/* eq_magnitude_response, lib.rs:99-150 (legacy (freq, gain_db, q) x 10 bands) */
int af_eq_magnitude_response(const double *frequencies_hz, size_t n, const double bands[10][3],
                             double sample_rate, double *out_db);
/* eq_magnitude_response_v2, lib.rs:191-212 */
int af_eq_magnitude_response_v2(const double *frequencies_hz, size_t n,
                                const af_eq_band_config bands[10], double sample_rate,
                                double *out_db);
/* engine's configured EQ, target response: ParametricEQ::magnitude_response_db, eq.rs:511-527 */
int af_engine_eq_magnitude_response(const af_engine *e, const double *frequencies_hz, size_t n,
                                    double *out_db);

#ifdef __cplusplus
}
#endif
#endif /* AUDIOFORGE_MI_H */
