// tfrec_amd/csrc/capi_bursts.h -- the entry points of the five burst stages on the recorder's table: the meter, the
// envelope (6r), the clock (6s), the track (6t, with its centres; 6v, its amplitude mode, with its levels; 6w, its auto-centre mode, with its centre records; 6x, its phase mode; 6y, its line code; 6z, its frame check) and the sync (6u).  What they share comes first -- the enables'
// preflight, the rebase of start_sample, the record-only reader and the record-plus-bitmap reader --, then each
// stage's enable and read, which add their own argument checks and buffers.  Included by capi.hip, which lists what is where.
#pragma once

// A stage's nouns in the messages: the stage, its records, its enable call
struct StageNames {
	const char *stage, *rec, *enable;
};
constexpr StageNames kMeterNames = { "burst meter", "burst", "tfrec_amd_enable_burst_meter" };
constexpr StageNames kEnvelopeNames = { "burst envelope", "envelope", "tfrec_amd_enable_burst_envelope" };
constexpr StageNames kClockNames = { "burst clock", "clock", "tfrec_amd_enable_burst_clock" };
constexpr StageNames kTrackNames = { "burst track", "track", "tfrec_amd_enable_burst_track" };
constexpr StageNames kCentreNames = { "auto-centre track", "centre", "tfrec_amd_enable_burst_track_auto" };
constexpr StageNames kCodeNames = { "line code", "code", "tfrec_amd_enable_burst_code" };
constexpr StageNames kCrcNames = { "frame check", "crc", "tfrec_amd_enable_burst_crc" };
constexpr StageNames kSyncNames = { "burst sync", "sync", "tfrec_amd_enable_burst_sync" };

// What every enable checks behind its own arguments, in this order: what the stage works on (`needs`, switched on by
// `needs_call`) is on, the stage is not, the stage's own limit (`limit`: what it needs, where the context lacks it), the context
// is live and no submit has been made; then the device is current.  The caller's EnableGuard comes behind it.
static int enable_preflight(tfrec_amd_ctx *c, const StageNames &nm, bool needs_on, const char *needs, const char *needs_call, bool on,
			    const char *limit = nullptr)
{
	if (!needs_on) {
		snprintf(g_err, sizeof(g_err), "the %s works on %s: call %s first", nm.stage, needs, needs_call);
		return TFREC_AMD_E_INVAL;
	}
	if (on) {
		snprintf(g_err, sizeof(g_err), "the %s is enabled already", nm.stage);
		return TFREC_AMD_E_INVAL;
	}
	if (limit) {
		snprintf(g_err, sizeof(g_err), "the %s needs %s", nm.stage, limit);
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->submitted) {
		snprintf(g_err, sizeof(g_err), "the %s is enabled before the first submit", nm.stage);
		return TFREC_AMD_E_STATE;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	return TFREC_AMD_OK;
}
static int recorder_preflight(tfrec_amd_ctx *c, const StageNames &nm, bool on, const char *limit = nullptr)
{
	return enable_preflight(c, nm, c->cap.lane.on, "the recorder's table", "tfrec_amd_enable_capture", on, limit);
}

// The record-only enable: the preflight and the sets' records
template <class Rec>
static int enable_run_records(tfrec_amd_ctx *c, RunRecords<Rec> &recs, const StageNames &nm, const char *limit = nullptr)
{
	TRY(recorder_preflight(c, nm, recs.on, limit));
	EnableGuard<RunRecords<Rec>> guard(c, recs);
	for (int k = 0; k < kSets; k++)
		TRY(own_device(c, recs.d_recs[k], (size_t)c->cap.max_runs * sizeof(Rec)));
	recs.on = guard.ok = true;
	return TFREC_AMD_OK;
}

// start_sample counts from the stream's last restart, as the table's does
template <class Rec>
static void rebase_start_samples(const tfrec_amd_ctx *c, int set, Rec *recs, size_t n)
{
	const std::vector<long long> &org = c->restart.set_origin[set];  // (empty: no submit before the set's one carried a reset)
	for (size_t i = 0; i < n; i++)
		if (recs[i].stream < org.size())
			recs[i].start_sample -= org[recs[i].stream];
}

// A read's start: the stage is on, the oldest submit's set on the recorder's lane is complete, its header
template <class Rec>
static int begin_records_read(tfrec_amd_ctx *c, const RunRecords<Rec> &recs, const StageNames &nm, int *set, CaptureHeader *hdr)
{
	if (!recs.on) {
		snprintf(g_err, sizeof(g_err), "the %s is off: call %s before the first submit", nm.stage, nm.enable);
		return TFREC_AMD_E_INVAL;
	}
	TRY(begin_side_read(c, c->cap.lane, "recorder", "call tfrec_amd_enable_capture before the first submit", set));
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[*set]));  // (behind the lane's written[set])
	HIPCHK(hipMemcpy(hdr, c->cap.d_hdr[*set], sizeof(*hdr), hipMemcpyDeviceToHost));
	return TFREC_AMD_OK;
}

// The record-only read (meter, envelope, clock).  Every entry of the table has a record, whatever the pool held: these stages
// read the decimated samples and the mask, not the pool.
template <class Rec>
static int read_run_records(tfrec_amd_ctx *c, const RunRecords<Rec> &recs, const StageNames &nm, Rec *out, size_t cap_runs, uint32_t *n_runs)
{
	if (!n_runs || (cap_runs > 0 && !out))
		return TFREC_AMD_E_INVAL;
	int set = 0;
	CaptureHeader hdr;
	TRY(begin_records_read(c, recs, nm, &set, &hdr));
	const size_t have = (size_t)std::min<unsigned long long>(hdr.n_runs, c->cap.max_runs);
	*n_runs = (uint32_t)std::min<unsigned long long>(hdr.n_runs, 0xffffffffull);
	if (cap_runs < have) {
		snprintf(g_err, sizeof(g_err), "room for %zu %s records, the submit delivers %zu", cap_runs, nm.rec, have);
		return TFREC_AMD_E_INVAL;
	}
	if (have)
		HIPCHK(hipMemcpy(out, recs.d_recs[set], have * sizeof(Rec), hipMemcpyDeviceToHost));
	rebase_start_samples(c, set, out, have);
	return hdr.n_runs > c->cap.max_runs ? TFREC_AMD_E_OVERFLOW : TFREC_AMD_OK;
}

// The record-plus-bitmap read (track, sync).  A record for every entry of the table; the words of the pairs
// tfrec_amd_read_captures delivers: on an overflow the prefix of whole runs that fit the pool, found on the records' own bit_offset
// and n_samples.  words == null asks for the counts and the records alone.
template <class Rec>
static int read_run_bitmaps(tfrec_amd_ctx *c, const RunRecords<Rec> &recs, uint32_t *const *d_words, const StageNames &nm, Rec *out,
			    size_t cap_runs, uint32_t *n_runs, uint32_t *words, size_t cap_words, uint64_t *n_words)
{
	if (!n_runs || !n_words || (cap_runs > 0 && !out) || (cap_words > 0 && !words))
		return TFREC_AMD_E_INVAL;
	int set = 0;
	CaptureHeader hdr;
	TRY(begin_records_read(c, recs, nm, &set, &hdr));
	const CaptureOut &o = c->cap;
	const bool overflow = hdr.n_runs > o.max_runs || hdr.n_pairs > o.max_samples;
	const size_t have = (size_t)std::min<unsigned long long>(hdr.n_runs, o.max_runs);
	std::vector<Rec> tmp(have);
	if (have)
		HIPCHK(hipMemcpy(tmp.data(), recs.d_recs[set], have * sizeof(Rec), hipMemcpyDeviceToHost));
	uint64_t pairs = hdr.n_pairs;
	if (overflow) {
		pairs = 0;
		for (size_t k = 0; k < have && tmp[k].bit_offset + tmp[k].n_samples <= o.max_samples; k++)
			pairs = tmp[k].bit_offset + tmp[k].n_samples;
	}
	const uint64_t nw = (pairs + 31) >> 5;
	*n_runs = (uint32_t)std::min<unsigned long long>(hdr.n_runs, 0xffffffffull);
	*n_words = nw;
	if (cap_runs < have || (words && cap_words < nw)) {
		snprintf(g_err, sizeof(g_err), "room for %zu %s records and %zu words, the submit delivers %zu and %llu", cap_runs, nm.rec, cap_words, have,
			 (unsigned long long)nw);
		return TFREC_AMD_E_INVAL;
	}
	rebase_start_samples(c, set, tmp.data(), have);
	if (words && nw)
		HIPCHK(hipMemcpy(words, d_words[set], (size_t)nw * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (have)
		memcpy(out, tmp.data(), have * sizeof(Rec));
	return overflow ? TFREC_AMD_E_OVERFLOW : TFREC_AMD_OK;
}

// ---- the meter, the envelope, the clock
int tfrec_amd_enable_burst_meter(tfrec_amd_ctx *c) { return c ? enable_run_records(c, c->burst, kMeterNames) : TFREC_AMD_E_INVAL; }
int tfrec_amd_read_bursts(tfrec_amd_ctx *c, tfrec_amd_burst *out, size_t cap_runs, uint32_t *n_runs)
{
	return c ? read_run_records(c, c->burst, kMeterNames, out, cap_runs, n_runs) : TFREC_AMD_E_INVAL;
}

int tfrec_amd_enable_burst_envelope(tfrec_amd_ctx *c) { return c ? enable_run_records(c, c->env, kEnvelopeNames) : TFREC_AMD_E_INVAL; }
int tfrec_amd_read_burst_envelopes(tfrec_amd_ctx *c, tfrec_amd_envelope *out, size_t cap_runs, uint32_t *n_runs)
{
	return c ? read_run_records(c, c->env, kEnvelopeNames, out, cap_runs, n_runs) : TFREC_AMD_E_INVAL;
}

int tfrec_amd_enable_burst_clock(tfrec_amd_ctx *c)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	// 8 segments a block: a record's device-side sums stay below 2^15 segments
	return enable_run_records(c, c->clk, kClockNames, c->cfg.max_blocks >= 4096 ? "max_blocks < 4096" : nullptr);
}
int tfrec_amd_read_burst_clocks(tfrec_amd_ctx *c, tfrec_amd_clock *out, size_t cap_runs, uint32_t *n_runs)
{
	return c ? read_run_records(c, c->clk, kClockNames, out, cap_runs, n_runs) : TFREC_AMD_E_INVAL;
}

// ---- the track
constexpr int kTrackCentreLimit = 192000;  // |hz| <= half the 384 kS/s channel rate
constexpr int kTrackLevelLimit = 65535;    // the amplitude mode's level: the trigger's unit, |I| + |Q|

// r = floor((8192 hz + 384000) / 768000) mod 4096, a true floor (|hz| <= 192000: the numerator stays inside 32 bits' worth of 64)
static int32_t track_index(int32_t hz)
{
	const long long a = 8192LL * hz + 384000, b = 768000;
	const long long q = a / b - ((a % b) < 0 ? 1 : 0);
	return (int32_t)(q & 4095);
}

constexpr int kTrackHeadMin = 64, kTrackHeadMax = 4096;  // the auto-centre mode's K
constexpr int kTrackLagMin = 1, kTrackLagMax = 64;        // the phase mode's m

// Every mode's enable: the frequency track (6t) or the amplitude track (6v), which differ in one kernel and in what idx holds, or
// the auto-centre track (6w: head = K != 0), whose idx holds the set centres in Hz and which adds its records and its carry, or the
// phase track (6x: head and lag = m != 0), which is the auto-centre's with 80 carried pairs per stream for its 16
static int enable_track(tfrec_amd_ctx *c, int32_t smooth, bool amplitude, int32_t head = 0, int32_t lag = 0)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	if (smooth < 1 || smooth > 16) {
		snprintf(g_err, sizeof(g_err), "the burst track's smooth is within [1, 16]");
		return TFREC_AMD_E_INVAL;
	}
	if (head && (head < kTrackHeadMin || head > kTrackHeadMax)) {
		snprintf(g_err, sizeof(g_err), "the auto-centre track's head is within [%d, %d]", kTrackHeadMin, kTrackHeadMax);
		return TFREC_AMD_E_INVAL;
	}
	if (lag && (lag < kTrackLagMin || lag > kTrackLagMax)) {
		snprintf(g_err, sizeof(g_err), "the phase track's lag is within [%d, %d]", kTrackLagMin, kTrackLagMax);
		return TFREC_AMD_E_INVAL;
	}
	TRY(recorder_preflight(c, kTrackNames, c->trk.on));
	EnableGuard<BurstTrack> guard(c, c->trk);
	BurstTrack &o = c->trk;
	const size_t n = (size_t)c->cfg.n_streams;
	o.n_words = (size_t)((c->cap.max_samples + 31) >> 5);
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, o.d_recs[k], (size_t)c->cap.max_runs * sizeof(tfrec_amd_track)));
		TRY(own_device(c, o.d_words[k], o.n_words * sizeof(uint32_t)));
		TRY(own_device(c, o.d_idx[k], n * sizeof(int32_t)));
		TRY(own_pinned(c, o.h_idx[k], n * sizeof(int32_t)));
	}
	const size_t ahead = lag ? 80 : 16;  // the pairs a stream carries (track.h: kTrackAhead; phase.h: kPhaseAhead)
	TRY(own_device(c, o.d_carry, n * ahead * sizeof(uint32_t)));
	TRY(own_device(c, o.d_prior, n * sizeof(uint32_t)));
	HIPCHK(hipMemset(o.d_carry, 0, n * ahead * sizeof(uint32_t)));  // (never used before a submit has written them: no first submit CONTINUES)
	HIPCHK(hipMemset(o.d_prior, 0, n * sizeof(uint32_t)));
	if (head) {
		for (int k = 0; k < kSets; k++)
			TRY(own_device(c, o.cen.d_recs[k], (size_t)c->cap.max_runs * sizeof(tfrec_amd_track_centre)));
		TRY(own_device(c, o.d_ccarry, n * sizeof(int2)));
		HIPCHK(hipMemset(o.d_ccarry, 0xff, n * sizeof(int2)));  // index -1: nothing carried
		o.head = head;
		o.lag = lag;
		o.cen.on = true;
	}
	o.idx.assign(n, 0);
	o.smooth = smooth;
	o.amplitude = amplitude;
	o.on = guard.ok = true;
	return TFREC_AMD_OK;
}
int tfrec_amd_enable_burst_track(tfrec_amd_ctx *c, int32_t smooth) { return enable_track(c, smooth, false); }
int tfrec_amd_enable_burst_track_amplitude(tfrec_amd_ctx *c, int32_t smooth) { return enable_track(c, smooth, true); }
int tfrec_amd_enable_burst_track_auto(tfrec_amd_ctx *c, int32_t smooth, int32_t head)
{
	if (c && !head) {  // (0 is enable_track's "no head")
		snprintf(g_err, sizeof(g_err), "the auto-centre track's head is within [%d, %d]", kTrackHeadMin, kTrackHeadMax);
		return TFREC_AMD_E_INVAL;
	}
	return enable_track(c, smooth, false, head);
}
int tfrec_amd_enable_burst_track_phase(tfrec_amd_ctx *c, int32_t smooth, int32_t head, int32_t lag)
{
	if (c && (!head || !lag)) {  // (0 is enable_track's "no head" and "no lag")
		snprintf(g_err, sizeof(g_err), "the phase track's head is within [%d, %d], its lag within [%d, %d]", kTrackHeadMin, kTrackHeadMax, kTrackLagMin,
			 kTrackLagMax);
		return TFREC_AMD_E_INVAL;
	}
	return enable_track(c, smooth, false, head, lag);
}

int tfrec_amd_set_burst_track_centre(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *hz, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !hz)))
		return TFREC_AMD_E_INVAL;
	if (!c->trk.on) {
		snprintf(g_err, sizeof(g_err), "the burst track is off: call tfrec_amd_enable_burst_track before the first submit");
		return TFREC_AMD_E_INVAL;
	}
	if (c->trk.amplitude) {
		snprintf(g_err, sizeof(g_err), "the burst track is the amplitude's: it has levels (tfrec_amd_set_burst_track_level), no centres");
		return TFREC_AMD_E_INVAL;
	}
	for (int i = 0; i < n; i++) {
		TRY(check_stream(c, streams[i]));
		if (hz[i] < -kTrackCentreLimit || hz[i] > kTrackCentreLimit) {
			snprintf(g_err, sizeof(g_err), "the burst track's centre %d Hz outside [-%d, %d]", (int)hz[i], kTrackCentreLimit, kTrackCentreLimit);
			return TFREC_AMD_E_INVAL;
		}
	}
	TRY(check_live(c));
	for (int i = 0; i < n; i++)
		c->trk.idx[streams[i]] = c->trk.cen.on ? hz[i] : track_index(hz[i]);  // (auto-centre mode: the fallback, in Hz)
	return TFREC_AMD_OK;
}

int tfrec_amd_set_burst_track_level(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *level, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !level)))
		return TFREC_AMD_E_INVAL;
	if (!c->trk.on || !c->trk.amplitude) {
		snprintf(g_err, sizeof(g_err), "the amplitude track is off: call tfrec_amd_enable_burst_track_amplitude before the first submit");
		return TFREC_AMD_E_INVAL;
	}
	for (int i = 0; i < n; i++) {
		TRY(check_stream(c, streams[i]));
		if (level[i] < 0 || level[i] > kTrackLevelLimit) {
			snprintf(g_err, sizeof(g_err), "the amplitude track's level %d outside [0, %d]", (int)level[i], kTrackLevelLimit);
			return TFREC_AMD_E_INVAL;
		}
	}
	TRY(check_live(c));
	for (int i = 0; i < n; i++)
		c->trk.idx[streams[i]] = level[i];
	return TFREC_AMD_OK;
}

int tfrec_amd_read_burst_tracks(tfrec_amd_ctx *c, tfrec_amd_track *out, size_t cap_runs, uint32_t *n_runs, uint32_t *words, size_t cap_words,
				uint64_t *n_words)
{
	return c ? read_run_bitmaps(c, c->trk, c->trk.d_words, kTrackNames, out, cap_runs, n_runs, words, cap_words, n_words) : TFREC_AMD_E_INVAL;
}

int tfrec_amd_read_burst_track_centres(tfrec_amd_ctx *c, tfrec_amd_track_centre *out, size_t cap_runs, uint32_t *n_runs)
{
	return c ? read_run_records(c, c->trk.cen, kCentreNames, out, cap_runs, n_runs) : TFREC_AMD_E_INVAL;
}

// ---- the sync
constexpr int kSyncSpanLimit = 2047;  // the track bits a stream carries from submit to submit

int tfrec_amd_enable_burst_sync(tfrec_amd_ctx *c, int32_t rate, uint64_t pattern, int32_t n_bits, int32_t max_errors, uint32_t flags)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	if (rate < 1000 || rate > 96000) {
		snprintf(g_err, sizeof(g_err), "the burst sync's rate is within [1000, 96000] bit/s");
		return TFREC_AMD_E_INVAL;
	}
	if (n_bits < 8 || n_bits > 64) {
		snprintf(g_err, sizeof(g_err), "the burst sync's pattern has 8 .. 64 bits");
		return TFREC_AMD_E_INVAL;
	}
	if (max_errors < 0 || 2 * (long long)max_errors >= n_bits) {
		snprintf(g_err, sizeof(g_err), "the burst sync's errors are within 0 <= E < n_bits / 2");
		return TFREC_AMD_E_INVAL;
	}
	if (flags & ~TFREC_AMD_SYNC_BOTH) {
		snprintf(g_err, sizeof(g_err), "the burst sync's flags are 0 or 1, the complemented word too");
		return TFREC_AMD_E_INVAL;
	}
	const long long span = (768000LL * (n_bits - 1) + rate) / (2LL * rate);
	if (span > kSyncSpanLimit) {
		snprintf(g_err, sizeof(g_err), "the burst sync's pattern spans %lld samples at %d bit/s, more than %d", span, (int)rate, kSyncSpanLimit);
		return TFREC_AMD_E_INVAL;
	}
	TRY(enable_preflight(c, kSyncNames, c->trk.on, "the burst track", "tfrec_amd_enable_burst_track", c->syn.on));
	EnableGuard<BurstSync> guard(c, c->syn);
	BurstSync &o = c->syn;
	const size_t n = (size_t)c->cfg.n_streams;
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, o.d_recs[k], (size_t)c->cap.max_runs * sizeof(tfrec_amd_burst_sync)));
		TRY(own_device(c, o.d_words[k], c->trk.n_words * sizeof(uint32_t)));
	}
	TRY(own_device(c, o.d_carry, n * 64 * sizeof(uint32_t)));
	TRY(own_device(c, o.d_hist, n * sizeof(uint32_t)));
	HIPCHK(hipMemset(o.d_carry, 0, n * 64 * sizeof(uint32_t)));  // (never used before a submit has written them: no first submit CONTINUES)
	HIPCHK(hipMemset(o.d_hist, 0, n * sizeof(uint32_t)));
	o.rate = rate;
	o.n_bits = n_bits;
	o.max_errors = max_errors;
	o.flags = flags;
	o.pattern = n_bits == 64 ? pattern : pattern & ((1ull << n_bits) - 1ull);
	o.on = guard.ok = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_read_burst_syncs(tfrec_amd_ctx *c, tfrec_amd_burst_sync *out, size_t cap_runs, uint32_t *n_runs, uint32_t *words, size_t cap_words,
			       uint64_t *n_words)
{
	return c ? read_run_bitmaps(c, c->syn, c->syn.d_words, kSyncNames, out, cap_runs, n_runs, words, cap_words, n_words) : TFREC_AMD_E_INVAL;
}

// ---- the line code
int tfrec_amd_enable_burst_code(tfrec_amd_ctx *c, int32_t rate, uint32_t taps, uint32_t flags)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	if (rate < 1000 || rate > 96000) {
		snprintf(g_err, sizeof(g_err), "the line code's rate is within [1000, 96000] bit/s");
		return TFREC_AMD_E_INVAL;
	}
	if (!taps) {
		snprintf(g_err, sizeof(g_err), "the line code has at least one tap");
		return TFREC_AMD_E_INVAL;
	}
	if (flags & ~TFREC_AMD_CODE_INVERT) {
		snprintf(g_err, sizeof(g_err), "the line code's flags are 0 or 1, the complemented output");
		return TFREC_AMD_E_INVAL;
	}
	const int top = 32 - __builtin_clz(taps);  // the highest tap's delay in symbols
	const long long span = (768000LL * top + rate) / (2LL * rate);
	if (span > kSyncSpanLimit) {
		snprintf(g_err, sizeof(g_err), "the line code's taps span %lld samples at %d bit/s, more than %d", span, (int)rate, kSyncSpanLimit);
		return TFREC_AMD_E_INVAL;
	}
	TRY(enable_preflight(c, kCodeNames, c->trk.on, "the burst track", "tfrec_amd_enable_burst_track", c->code.on));
	EnableGuard<BurstCode> guard(c, c->code);
	BurstCode &o = c->code;
	const size_t n = (size_t)c->cfg.n_streams;
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, o.d_recs[k], (size_t)c->cap.max_runs * sizeof(tfrec_amd_track)));
		TRY(own_device(c, o.d_words[k], c->trk.n_words * sizeof(uint32_t)));
	}
	TRY(own_device(c, o.d_carry, n * 64 * sizeof(uint32_t)));
	TRY(own_device(c, o.d_hist, n * sizeof(uint32_t)));
	HIPCHK(hipMemset(o.d_carry, 0, n * 64 * sizeof(uint32_t)));  // (never used before a submit has written them: no first submit CONTINUES)
	HIPCHK(hipMemset(o.d_hist, 0, n * sizeof(uint32_t)));
	o.rate = rate;
	o.taps = taps;
	o.flags = flags;
	o.on = guard.ok = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_read_burst_codes(tfrec_amd_ctx *c, tfrec_amd_track *out, size_t cap_runs, uint32_t *n_runs, uint32_t *words, size_t cap_words,
			       uint64_t *n_words)
{
	return c ? read_run_bitmaps(c, c->code, c->code.d_words, kCodeNames, out, cap_runs, n_runs, words, cap_words, n_words) : TFREC_AMD_E_INVAL;
}

// ---- the frame check
int tfrec_amd_enable_burst_crc(tfrec_amd_ctx *c, int32_t rate, int32_t n_bytes, int32_t skip, int32_t width, uint32_t poly, uint32_t init,
			       uint32_t xorout, uint32_t flags)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	const tfrec_crc::Settings st = { rate, n_bytes, skip, width, poly, init, xorout, flags };
	if (const char *why = tfrec_crc::refusal(st)) {
		snprintf(g_err, sizeof(g_err), "%s", why);
		return TFREC_AMD_E_INVAL;
	}
	TRY(enable_preflight(c, kCrcNames, c->trk.on, "the burst track", "tfrec_amd_enable_burst_track", c->crc.on));
	EnableGuard<BurstCrc> guard(c, c->crc);
	BurstCrc &o = c->crc;
	const size_t n = (size_t)c->cfg.n_streams;
	std::vector<tfrec_crc::Term> terms;
	uint32_t r0 = 0;
	tfrec_crc::build(st, terms, r0);
	static_assert(sizeof(tfrec_crc::Term) == sizeof(uint2), "crc_kernel reads a term as a uint2 (off, col)");
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, o.d_recs[k], (size_t)c->cap.max_runs * sizeof(tfrec_amd_burst_crc)));
		TRY(own_device(c, o.d_words[k], c->trk.n_words * sizeof(uint32_t)));
	}
	TRY(own_device(c, o.d_carry, n * 512 * sizeof(uint32_t)));
	TRY(own_device(c, o.d_hist, n * sizeof(uint32_t)));
	TRY(own_device(c, o.d_terms, (size_t)8 * (size_t)n_bytes * sizeof(uint2)));
	HIPCHK(hipMemset(o.d_carry, 0, n * 512 * sizeof(uint32_t)));  // (never used before a submit has written them: no first submit CONTINUES)
	HIPCHK(hipMemset(o.d_hist, 0, n * sizeof(uint32_t)));
	HIPCHK(hipMemset(o.d_terms, 0, (size_t)8 * (size_t)n_bytes * sizeof(uint2)));
	if (!terms.empty())
		HIPCHK(hipMemcpy(o.d_terms, terms.data(), terms.size() * sizeof(uint2), hipMemcpyHostToDevice));
	o.reach = (int)tfrec_crc::reach(st);
	o.width = width;
	o.n_terms = (int)terms.size();
	o.r0 = r0;
	o.on = guard.ok = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_read_burst_crcs(tfrec_amd_ctx *c, tfrec_amd_burst_crc *out, size_t cap_runs, uint32_t *n_runs, uint32_t *words, size_t cap_words,
			      uint64_t *n_words)
{
	return c ? read_run_bitmaps(c, c->crc, c->crc.d_words, kCrcNames, out, cap_runs, n_runs, words, cap_words, n_words) : TFREC_AMD_E_INVAL;
}
