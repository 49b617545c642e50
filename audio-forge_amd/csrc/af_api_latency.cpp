// af_api_latency.cpp -- the C ABI of the latency calibration (af_latency_*): python/mic_eq/analysis/latency_calibration.py's
// analyze_latency for a batch of recordings.  The host half: the probe's burst and offsets (_coded_probe_components, :74-115),
// the per-stream search windows and early exits (:253-345), the grouping of the streams by transform length, and, when the
// results are read, the rules of :424-515 (af_latency_math.h's lm_fold).  The kernels are af_latency.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <map>
#include <vector>

#include "af_api_internal.hpp"
#include "af_latency_host.hpp"

struct af_latency {
  int device = 0;
  double sample_rate = 48000.0;
  int32_t max_streams = 0;
  int64_t max_record = 0;
  bool touched_device = false;
  std::vector<double> probe, burst;  // centred (:276) / as _coded_probe_components leaves it
  double probe_energy = 0.0, burst_energy = 0.0;
  std::vector<int32_t> offsets;
  int32_t local_radius = 0;
  std::vector<double2> twiddle;
  // the last analysis
  int32_t n_streams = 0;
  std::vector<lm_search> searches;
  std::vector<int32_t> lengths;
  std::vector<af::LatencyJob> jobs;
  int64_t prefix_stride = 0, full_stride = 0;
  int32_t burst_cap = 0;
  af::DeviceBuffer<float> d_rec;
  af::DeviceBuffer<double> d_probe, d_burst, d_prefix, d_full, d_bursts, d_phat;
  af::DeviceBuffer<double2> d_twiddle, d_work0, d_work1;
  af::DeviceBuffer<int32_t> d_lengths, d_streams;
  af::DeviceBuffer<af::LatencyJob> d_jobs;
  af::DeviceBuffer<af::LatencySearchLags> d_search;
  af::DeviceBuffer<lm_record> d_records;
  std::map<int, af::DeviceBuffer<double2>> d_spectra;  // rfft(burst, n) by log2 of the complex length
  af::EventChain spans;

  ~af_latency() {
    if (touched_device) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
  }
};

namespace {

const double kBarker13[13] = {1.0, 1.0, 1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0};  // :17-20
const double kPi = 3.141592653589793;

int ceil_log2(int64_t v) {
  int b = 0;
  while (((int64_t)1 << b) < v) ++b;
  return b;
}

// _coded_probe_components, :74-115, with DEFAULT_REPETITIONS
void coded_probe_components(double sample_rate, int64_t total, std::vector<double> *burst, std::vector<int32_t> *offsets) {
  const int64_t repetitions = LM_MAX_OFFSETS;
  int64_t chip = std::max<int64_t>(4, (int64_t)std::rint(sample_rate * 0.0005));
  const int64_t min_spacing = std::max<int64_t>(chip, (int64_t)std::rint(sample_rate * 0.006));
  while (chip > 4) {
    if (repetitions * 13 * chip + (repetitions - 1) * min_spacing <= total) break;
    --chip;
  }
  const int64_t M = 13 * chip;
  std::vector<double> b((size_t)M);
  for (int64_t i = 0; i < M; ++i)  // np.hanning: 0.5 + 0.5 cos(pi n / (M - 1)), n = 1 - M, 3 - M, ...
    b[(size_t)i] = kBarker13[i / chip] * (0.5 + 0.5 * std::cos(kPi * (double)(1 - M + 2 * i) / (double)(M - 1)));
  const double mean = lm_sum(b.data(), M) / (double)M;
  double peak = 0.0;
  for (double &v : b) { v -= mean; peak = std::max(peak, std::fabs(v)); }
  if (peak > 0.0)
    for (double &v : b) v /= peak;
  offsets->clear();
  if (total <= M) {
    b.resize((size_t)total);
    offsets->push_back(0);
  } else {
    const int64_t spacing = std::max(min_spacing, std::max<int64_t>(0, total - repetitions * M) / (repetitions - 1));
    for (int64_t r = 0, cursor = 0; r < repetitions && cursor + M <= total; ++r, cursor += M + spacing) offsets->push_back((int32_t)cursor);
    if (offsets->empty()) offsets->push_back(0);
  }
  *burst = std::move(b);
}

double energy_of(const std::vector<double> &v) {  // float(np.sum(ref * ref) + 1e-12), :160
  std::vector<double> sq(v.size());
  for (size_t i = 0; i < v.size(); ++i) sq[i] = v[i] * v[i];
  return lm_sum(sq.data(), (int64_t)sq.size()) + 1e-12;
}

// np.fft.rfft(burst, n) for n = 2^(log_n + 1) on the host: radix 2 with the object's twiddle table
std::vector<double2> burst_spectrum(const af_latency *h, int log_n) {
  const int bits = log_n + 1;
  const size_t n = (size_t)1 << bits;
  std::vector<std::complex<double>> z(n, 0.0);
  for (size_t i = 0; i < h->burst.size() && i < n; ++i) {
    size_t r = 0;
    for (int b = 0; b < bits; ++b) r |= ((i >> b) & 1) << (bits - 1 - b);
    z[r] = h->burst[i];
  }
  for (int st = 1; st <= bits; ++st) {
    const size_t half = (size_t)1 << (st - 1);
    for (size_t i0 = 0; i0 < n; i0 += 2 * half)
      for (size_t j = 0; j < half; ++j) {
        const double2 t = h->twiddle[j << (af::kLatLogTable - st)];
        const std::complex<double> w(t.x, t.y), u = z[i0 + j], v = z[i0 + j + half] * w;
        z[i0 + j] = u + v;
        z[i0 + j + half] = u - v;
      }
  }
  std::vector<double2> out(n / 2 + 1);
  for (size_t k = 0; k <= n / 2; ++k) out[k] = double2{z[k].real(), z[k].imag()};
  return out;
}

int ensure_constants(af_latency *h) {
  if (h->d_twiddle.get()) return AF_OK;
  AF_HIP(h->d_probe.reserve_exact(sizeof(double) * h->probe.size()));
  AF_HIP(h->d_burst.reserve_exact(sizeof(double) * h->burst.size()));
  AF_HIP(hipMemcpy(h->d_probe, h->probe.data(), sizeof(double) * h->probe.size(), hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(h->d_burst, h->burst.data(), sizeof(double) * h->burst.size(), hipMemcpyHostToDevice));
  AF_HIP(h->d_twiddle.reserve_exact(sizeof(double2) * h->twiddle.size()));
  AF_HIP(h->d_twiddle.keep_if(hipMemcpy(h->d_twiddle, h->twiddle.data(), sizeof(double2) * h->twiddle.size(), hipMemcpyHostToDevice)));
  return AF_OK;
}

int ensure_spectrum(af_latency *h, int log_n) {
  af::DeviceBuffer<double2> &buf = h->d_spectra[log_n];
  if (buf.get()) return AF_OK;
  const std::vector<double2> spectrum = burst_spectrum(h, log_n);
  AF_HIP(buf.reserve_exact(sizeof(double2) * spectrum.size()));
  AF_HIP(buf.keep_if(hipMemcpy(buf, spectrum.data(), sizeof(double2) * spectrum.size(), hipMemcpyHostToDevice)));
  return AF_OK;
}

af::LatencyArgs base_args(const af_latency *h) {
  af::LatencyArgs a{};
  a.probe = h->d_probe;
  a.burst = h->d_burst;
  a.probe_len = (int32_t)h->probe.size();
  a.burst_len = (int32_t)h->burst.size();
  a.probe_energy = h->probe_energy;
  a.burst_energy = h->burst_energy;
  a.n_offsets = (int32_t)h->offsets.size();
  a.local_radius = h->local_radius;
  for (size_t k = 0; k < h->offsets.size(); ++k) a.offsets[k] = h->offsets[k];
  return a;
}

int la_analyze(af_latency *h, const float *recorded, bool on_device, int64_t n, int64_t stride, int32_t S, const int64_t *lengths,
               const af_latency_search *search) {
  if (!h || !recorded || !search) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (S < 1 || S > h->max_streams) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be in 1..%d", h->max_streams);
  if (n < 1 || n > h->max_record)
    return fail(AF_ERR_INVALID_ARGUMENT, "n_samples must be in 1..%lld (max_record_samples)", (long long)h->max_record);
  if (stride < n) return fail(AF_ERR_INVALID_ARGUMENT, "stride must cover n_samples");
  for (int32_t s = 0; s < S; ++s) {
    if (lengths && (lengths[s] < 0 || lengths[s] > n))
      return fail(AF_ERR_INVALID_ARGUMENT, "lengths[%d] = %lld is outside 0..n_samples", s, (long long)lengths[s]);
    const af_latency_search &q = search[s];
    const double values[6] = {q.min_search_ms, q.max_search_ms, q.has_playback_start ? q.expected_playback_start_ms : 0.0,
                              q.has_playback_jitter ? q.expected_playback_jitter_ms : 0.0,
                              q.has_latency_min ? q.expected_latency_min_ms : 0.0, q.has_latency_max ? q.expected_latency_max_ms : 0.0};
    for (double v : values)
      if (!std::isfinite(v)) return fail(AF_ERR_INVALID_ARGUMENT, "search[%d]: every search value must be finite", s);
  }
  const int64_t m = (int64_t)h->probe.size(), bl = (int64_t)h->burst.size();
  h->n_streams = 0;
  h->searches.assign((size_t)S, lm_search{});
  h->lengths.assign((size_t)S, 0);
  h->jobs.assign((size_t)S * af::kLatJobs, af::LatencyJob{0, 0});
  std::vector<af::LatencySearchLags> lags((size_t)S);
  std::map<int, std::vector<int32_t>> groups;
  int64_t longest = 0, full_cap = 0;
  for (int32_t s = 0; s < S; ++s) {
    const int64_t len = lengths ? lengths[s] : n;
    const lm_search q = lm_search_from(&search[s], h->sample_rate, len, m);
    h->searches[(size_t)s] = q;
    lags[(size_t)s] = af::LatencySearchLags{q.min_lag, q.max_lag};
    if (q.exit_code != AF_LATENCY_EXIT_NONE) continue;
    const int64_t lo = std::max<int64_t>(q.min_lag, 0), hi = std::min<int64_t>(q.max_lag, len - m);
    h->lengths[(size_t)s] = (int32_t)len;
    h->jobs[(size_t)s * af::kLatJobs] = af::LatencyJob{(int32_t)lo, (int32_t)(hi - lo + 1)};
    longest = std::max(longest, len);
    full_cap = std::max(full_cap, hi - lo + 1);
    groups[std::max(ceil_log2(len + bl) - 1, 4)].push_back(s);
  }
  std::vector<int32_t> order;
  for (const auto &g : groups) order.insert(order.end(), g.second.begin(), g.second.end());

  AF_HIP(hipSetDevice(h->device));
  h->touched_device = true;
  AF_HIP(hipDeviceSynchronize());  // nothing of an earlier analysis still reads what is replaced
  if (int rc = ensure_constants(h); rc != AF_OK) return rc;
  size_t work_points = 0;
  for (const auto &g : groups) {
    if (int rc = ensure_spectrum(h, g.first); rc != AF_OK) return rc;
    if (g.first > af::kLatLdsLogMax) {
      const size_t points = (size_t)1 << g.first, fit = std::max<size_t>(1, af::kLatWorkspaceBytes / (2 * points * sizeof(double2)));
      work_points = std::max(work_points, points * std::min(fit, g.second.size()));
    }
  }
  const size_t f4 = sizeof(float), f8 = sizeof(double);
  const float *d_in = recorded;
  int64_t in_stride = stride;
  if (!on_device) {
    AF_HIP(h->d_rec.reserve_exact(f4 * (size_t)S * n));
    AF_HIP(hipMemcpy2D(h->d_rec, f4 * n, recorded, f4 * stride, f4 * n, S, hipMemcpyHostToDevice));
    d_in = h->d_rec;
    in_stride = n;
  }
  h->prefix_stride = longest + 1;
  h->full_stride = std::max<int64_t>(full_cap, 1);
  h->burst_cap = 2 * h->local_radius + 2;
  AF_HIP(h->d_prefix.reserve_exact(f8 * (size_t)S * h->prefix_stride));
  AF_HIP(h->d_full.reserve_exact(f8 * (size_t)S * h->full_stride));
  AF_HIP(h->d_bursts.reserve_exact(f8 * (size_t)S * LM_MAX_OFFSETS * h->burst_cap));
  AF_HIP(h->d_phat.reserve_exact(f8 * (size_t)S * LM_MAX_OFFSETS * h->burst_cap));
  AF_HIP(h->d_lengths.reserve_exact(sizeof(int32_t) * (size_t)S));
  AF_HIP(h->d_streams.reserve_exact(sizeof(int32_t) * (size_t)S));
  AF_HIP(h->d_jobs.reserve_exact(sizeof(af::LatencyJob) * h->jobs.size()));
  AF_HIP(h->d_search.reserve_exact(sizeof(af::LatencySearchLags) * (size_t)S));
  AF_HIP(h->d_records.reserve_exact(sizeof(lm_record) * (size_t)S));
  if (work_points) {
    AF_HIP(h->d_work0.reserve_exact(sizeof(double2) * work_points));
    AF_HIP(h->d_work1.reserve_exact(sizeof(double2) * work_points));
  }
  AF_HIP(hipMemcpy(h->d_lengths, h->lengths.data(), sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice));
  if (!order.empty()) AF_HIP(hipMemcpy(h->d_streams, order.data(), sizeof(int32_t) * order.size(), hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(h->d_jobs, h->jobs.data(), sizeof(af::LatencyJob) * h->jobs.size(), hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(h->d_search, lags.data(), sizeof(af::LatencySearchLags) * (size_t)S, hipMemcpyHostToDevice));
  AF_HIP(hipMemset(h->d_records, 0, sizeof(lm_record) * (size_t)S));

  af::LatencyArgs a = base_args(h);
  a.rec = d_in;
  a.stride = in_stride;
  a.length = h->d_lengths;
  a.records = h->d_records;
  a.jobs = h->d_jobs;
  a.search = h->d_search;
  a.prefix = h->d_prefix;
  a.prefix_stride = h->prefix_stride;
  a.full_scores = h->d_full;
  a.full_stride = h->full_stride;
  a.burst_scores = h->d_bursts;
  a.phat_corr = h->d_phat;
  a.burst_cap = h->burst_cap;
  a.n_streams = S;
  hipStream_t q = nullptr;
  // from here to the end nothing waits for the device: the burst windows go from the pick to the next launch in device memory
  h->spans.restart();
  AF_HIP(h->spans.mark(q));
  if (!order.empty()) {
    AF_HIP(af::launch_latency_condition(a, q));
    AF_HIP(h->spans.mark(q));
    AF_HIP(af::launch_latency_score(a, 0, (int32_t)full_cap, q));
    AF_HIP(af::launch_latency_pick(a, 0, q));
    AF_HIP(h->spans.mark(q));
    AF_HIP(af::launch_latency_score(a, 1, h->burst_cap, q));
    AF_HIP(af::launch_latency_pick(a, 1, q));
    AF_HIP(h->spans.mark(q));
    size_t at = 0;
    for (const auto &g : groups) {
      af::LatencyPhatArgs p{};
      p.log_n = g.first;
      p.twiddle = h->d_twiddle;
      p.burst_spectrum = h->d_spectra[g.first];
      p.work0 = h->d_work0;
      p.work1 = h->d_work1;
      const size_t points = (size_t)1 << g.first;
      const size_t fit = g.first > af::kLatLdsLogMax ? std::max<size_t>(1, af::kLatWorkspaceBytes / (2 * points * sizeof(double2))) : g.second.size();
      for (size_t done = 0; done < g.second.size(); done += fit) {  // tiles of the group that fit the workspace
        p.streams = h->d_streams.get() + at + done;
        p.n_group = (int32_t)std::min(fit, g.second.size() - done);
        AF_HIP(af::launch_latency_phat(a, p, q));
      }
      at += g.second.size();
    }
    AF_HIP(h->spans.mark(q));
  }
  h->n_streams = S;
  return AF_OK;
}

const char *const kExitText[AF_LATENCY_EXIT_COUNT] = {
    nullptr,
    "Unsupported latency route; expected output_to_input.",  // :263
    "Recording too short for reliable correlation.",         // :287
    "Search window is outside valid lag range.",             // :322
    "Search window does not overlap captured audio.",        // :344
    "Recording contains non-finite samples."};
const char *const kMessageText[AF_LATENCY_MESSAGE_COUNT] = {
    "ok", "Repeated probes disagree; echoes or bleed make latency ambiguous.",
    "Echo ambiguity: competing correlation peaks are too close.", "Low confidence or ambiguous coded-probe correlation."};  // :487-494

}  // namespace

extern "C" {

int af_latency_create(double sample_rate, const double *probe, int64_t probe_samples, int32_t max_streams, int64_t max_record_samples,
                      int32_t device, af_latency **out) {
  if (!out) return fail(AF_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  if (!std::isfinite(sample_rate) || sample_rate <= 0.0) return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be positive and finite");
  if (!probe) return fail(AF_ERR_INVALID_ARGUMENT, "probe is null");
  if (probe_samples < LM_MIN_PROBE) return fail(AF_ERR_INVALID_ARGUMENT, "probe_samples must be at least %d", LM_MIN_PROBE);
  if (probe_samples > AF_LATENCY_MAX_TRANSFORM) return fail(AF_ERR_INVALID_ARGUMENT, "probe_samples must be at most %d", AF_LATENCY_MAX_TRANSFORM);
  if (max_streams < 1) return fail(AF_ERR_INVALID_ARGUMENT, "max_streams must be positive");
  if (max_record_samples < 1) return fail(AF_ERR_INVALID_ARGUMENT, "max_record_samples must be positive");
  if (device < 0) return fail(AF_ERR_INVALID_ARGUMENT, "device must be >= 0");
  if (!af::check_finite(probe, 1, probe_samples, probe_samples)) return fail(AF_ERR_INVALID_ARGUMENT, "probe must contain only finite samples");
  if (sample_rate > 1.0e7) return fail(AF_ERR_INVALID_ARGUMENT, "sample_rate must be at most 1e7");
  af_latency *h = new af_latency();
  h->sample_rate = sample_rate;
  h->device = device;
  h->max_streams = max_streams;
  h->max_record = max_record_samples;
  const double mean = lm_sum(probe, probe_samples) / (double)probe_samples;  // _normalize_audio, :118-122
  h->probe.resize((size_t)probe_samples);
  for (int64_t i = 0; i < probe_samples; ++i) h->probe[(size_t)i] = probe[i] - mean;
  coded_probe_components(sample_rate, probe_samples, &h->burst, &h->offsets);
  if ((int64_t)h->burst.size() < LM_MIN_PROBE || h->offsets.empty()) {  // :326-328
    h->burst = h->probe;
    h->offsets.assign(1, 0);
  }
  h->probe_energy = energy_of(h->probe);
  h->burst_energy = energy_of(h->burst);
  h->local_radius = (int32_t)std::max<int64_t>((int64_t)std::rint(sample_rate * 0.010), (int64_t)h->burst.size());  // :351
  const int64_t transform = (int64_t)1 << ceil_log2(max_record_samples + (int64_t)h->burst.size());
  if (transform > AF_LATENCY_MAX_TRANSFORM) {
    const int64_t burst = (int64_t)h->burst.size();
    delete h;
    return fail(AF_ERR_INVALID_ARGUMENT,
                "max_record_samples + burst (%lld + %lld) needs a transform of %lld real points; at most %d are built (5.4 s at 48 kHz)",
                (long long)max_record_samples, (long long)burst, (long long)transform, AF_LATENCY_MAX_TRANSFORM);
  }
  const size_t half = (size_t)1 << (af::kLatLogTable - 1);
  h->twiddle.resize(half);
  for (size_t k = 0; k < half; ++k) {
    const long double angle = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)(2 * half);
    h->twiddle[k] = double2{(double)cosl(angle), (double)sinl(angle)};
  }
  *out = h;
  return AF_OK;
}

void af_latency_destroy(af_latency *h) { delete h; }

int af_latency_layout(af_latency *h, int32_t *n_offsets, int32_t *offsets, int32_t *burst_samples, int32_t *local_radius) {
  if (!h || !n_offsets || !offsets || !burst_samples || !local_radius) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  *n_offsets = (int32_t)h->offsets.size();
  for (size_t k = 0; k < h->offsets.size(); ++k) offsets[k] = h->offsets[k];
  *burst_samples = (int32_t)h->burst.size();
  *local_radius = h->local_radius;
  return AF_OK;
}

int af_latency_analyze_host(af_latency *h, const float *recorded, int64_t n_samples, int64_t stride, int32_t n_streams,
                            const int64_t *lengths, const af_latency_search *search) {
  return la_analyze(h, recorded, false, n_samples, stride, n_streams, lengths, search);
}

int af_latency_analyze_device(af_latency *h, const float *d_recorded, int64_t n_samples, int64_t stride, int32_t n_streams,
                              const int64_t *lengths, const af_latency_search *search) {
  return la_analyze(h, d_recorded, true, n_samples, stride, n_streams, lengths, search);
}

int af_latency_read_results(af_latency *h, af_latency_result *out, int32_t n_streams) {
  if (!h || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (h->n_streams == 0) return fail(AF_ERR_STATE, "no analysis has been made");
  if (n_streams != h->n_streams) return fail(AF_ERR_INVALID_ARGUMENT, "n_streams must be the last analysis's %d", h->n_streams);
  AF_HIP(hipSetDevice(h->device));
  std::vector<lm_record> records((size_t)n_streams);
  AF_HIP(hipMemcpy(records.data(), h->d_records, sizeof(lm_record) * records.size(), hipMemcpyDeviceToHost));
  for (int32_t s = 0; s < n_streams; ++s)
    lm_fold(records[(size_t)s], h->searches[(size_t)s], h->sample_rate, (int)h->offsets.size(), h->offsets.data(), &out[s]);
  return AF_OK;
}

int af_latency_read_scores(af_latency *h, int32_t stream, int32_t which, int32_t *lag_lo, int32_t *count, double *scores,
                           double *window_energy, int32_t *phat_lo, int32_t *phat_count, double *phat, int64_t capacity) {
  if (!h || !lag_lo || !count || !phat_lo || !phat_count) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (h->n_streams == 0) return fail(AF_ERR_STATE, "no analysis has been made");
  if (stream < 0 || stream >= h->n_streams) return fail(AF_ERR_INVALID_ARGUMENT, "stream must be in 0..%d", h->n_streams - 1);
  if (which < 0 || which > (int32_t)h->offsets.size()) return fail(AF_ERR_INVALID_ARGUMENT, "which must be in 0..%d", (int)h->offsets.size());
  *lag_lo = *count = *phat_lo = *phat_count = 0;
  if (h->lengths[(size_t)stream] == 0) return AF_OK;  // an early exit: nothing was scored
  AF_HIP(hipSetDevice(h->device));
  lm_record r;
  AF_HIP(hipMemcpy(&r, h->d_records.get() + stream, sizeof r, hipMemcpyDeviceToHost));
  if (r.non_finite) return AF_OK;
  const int k = which - 1;
  *lag_lo = which ? r.burst_lo[k] : h->jobs[(size_t)stream * af::kLatJobs].lo;
  *count = which ? r.burst_count[k] : r.full_count;
  if (which) { *phat_lo = r.phat_lo[k]; *phat_count = r.phat_count[k]; }
  if (*count > capacity || *phat_count > capacity) return fail(AF_ERR_INVALID_ARGUMENT, "capacity must hold %d values", std::max(*count, *phat_count));
  const double *d_scores = which ? h->d_bursts.get() + ((size_t)stream * LM_MAX_OFFSETS + k) * h->burst_cap
                                 : h->d_full.get() + (size_t)stream * h->full_stride;
  if (scores && *count) AF_HIP(hipMemcpy(scores, d_scores, sizeof(double) * *count, hipMemcpyDeviceToHost));
  if (window_energy && *count) {  // the difference of two values of the device's prefix, as the score kernel takes it
    const int64_t ref_len = which ? (int64_t)h->burst.size() : (int64_t)h->probe.size();
    std::vector<double> prefix((size_t)(*count + ref_len));
    AF_HIP(hipMemcpy(prefix.data(), h->d_prefix.get() + (size_t)stream * h->prefix_stride + *lag_lo, sizeof(double) * prefix.size(),
                     hipMemcpyDeviceToHost));
    for (int32_t i = 0; i < *count; ++i) window_energy[i] = prefix[(size_t)(i + ref_len)] - prefix[(size_t)i];
  }
  if (phat && *phat_count)
    AF_HIP(hipMemcpy(phat, h->d_phat.get() + ((size_t)stream * LM_MAX_OFFSETS + k) * h->burst_cap, sizeof(double) * *phat_count,
                     hipMemcpyDeviceToHost));
  return AF_OK;
}

int af_latency_last_kernel_ms(af_latency *h, double *ms, double *pass_ms) {
  if (!h || !ms) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  *ms = 0.0;
  if (pass_ms)
    for (int p = 0; p < AF_LATENCY_PASSES; ++p) pass_ms[p] = 0.0;
  if (h->n_streams == 0 || h->spans.marks() != AF_LATENCY_PASSES + 1) return AF_OK;
  AF_HIP(hipSetDevice(h->device));
  AF_HIP(h->spans.wait_last());
  AF_HIP(h->spans.elapsed(0, AF_LATENCY_PASSES, ms));
  if (pass_ms)
    for (int p = 0; p < AF_LATENCY_PASSES; ++p) AF_HIP(h->spans.elapsed((size_t)p, (size_t)p + 1, &pass_ms[p]));
  return AF_OK;
}

const char *af_latency_message_text(int32_t exit_code, int32_t message) {
  if (exit_code < 0 || exit_code >= AF_LATENCY_EXIT_COUNT) return nullptr;
  if (exit_code != AF_LATENCY_EXIT_NONE) return kExitText[exit_code];
  return message >= 0 && message < AF_LATENCY_MESSAGE_COUNT ? kMessageText[message] : nullptr;
}

int af_latency_debug_rfft(af_latency *h, const float *x, int64_t n_real, double *out) {
  if (!h || !x || !out) return fail(AF_ERR_INVALID_ARGUMENT, "null argument");
  if (n_real < 512 || n_real > AF_LATENCY_MAX_TRANSFORM || (n_real & (n_real - 1)))
    return fail(AF_ERR_INVALID_ARGUMENT, "n_real must be a power of two in 512..%d", AF_LATENCY_MAX_TRANSFORM);
  const int log_n = ceil_log2(n_real) - 1;
  const size_t points = (size_t)1 << log_n;
  AF_HIP(hipSetDevice(h->device));
  h->touched_device = true;
  AF_HIP(hipDeviceSynchronize());
  if (int rc = ensure_constants(h); rc != AF_OK) return rc;
  af::DeviceBuffer<float> d_x;
  af::DeviceBuffer<double2> d_out, w0, w1;
  af::DeviceBuffer<int32_t> d_ints;  // length, stream
  af::DeviceBuffer<lm_record> d_record;
  AF_HIP(d_x.reserve_exact(sizeof(float) * (size_t)n_real));
  AF_HIP(d_out.reserve_exact(sizeof(double2) * (points + 1)));
  AF_HIP(d_ints.reserve_exact(sizeof(int32_t) * 2));
  AF_HIP(d_record.reserve_exact(sizeof(lm_record)));
  if (log_n > af::kLatLdsLogMax) {
    AF_HIP(w0.reserve_exact(sizeof(double2) * points));
    AF_HIP(w1.reserve_exact(sizeof(double2) * points));
  }
  const int32_t ints[2] = {(int32_t)n_real, 0};
  AF_HIP(hipMemcpy(d_x, x, sizeof(float) * (size_t)n_real, hipMemcpyHostToDevice));
  AF_HIP(hipMemcpy(d_ints, ints, sizeof ints, hipMemcpyHostToDevice));
  AF_HIP(hipMemset(d_record, 0, sizeof(lm_record)));  // mean 0: the input as it is
  af::LatencyArgs a = base_args(h);
  a.rec = d_x;
  a.stride = n_real;
  a.length = d_ints;
  a.records = d_record;
  a.n_streams = 1;
  af::LatencyPhatArgs p{};
  p.streams = d_ints.get() + 1;
  p.n_group = 1;
  p.log_n = log_n;
  p.twiddle = h->d_twiddle;
  p.work0 = w0;
  p.work1 = w1;
  p.spectrum_out = d_out;
  AF_HIP(af::launch_latency_phat(a, p, nullptr));
  AF_HIP(hipMemcpy(out, d_out, sizeof(double2) * (points + 1), hipMemcpyDeviceToHost));
  return AF_OK;
}

}  // extern "C"
