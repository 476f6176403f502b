// tfrec_amd/csrc/capi_streams.h -- what restarts a stream: included by capi.hip, which lists what is where.
#pragma once

// a configure or a tune: from the next submit on the kernels read every stream's own settings
static void use_per_stream(tfrec_amd_ctx *c)
{
	if (c->settings.per_stream)
		return;
	c->settings.per_stream = true;
	c->launch.scfg = c->settings.d_scfg;
	c->taps.scfg = c->settings.d_scfg;
	for (int k = 0; k < 20; k++)  // f2: the narrow taps from now on (w: the wide ones)
		c->taps.f2[k][0] = c->taps.f2[k][1] = (float)kNarrowTaps[k] / 65536.0f;
}

// mark stream s to restart at the next submit (once per submit)
static void mark_restart(tfrec_amd_ctx *c, int32_t s)
{
	if (!c->restart.marked[s]) {
		c->restart.marked[s] = 1;
		c->restart.pending.push_back(s);
	}
}

int tfrec_amd_reset_streams(tfrec_amd_ctx *c, const int32_t *streams, int n)
{
	if (!c || n < 0 || (n > 0 && !streams))
		return TFREC_AMD_E_INVAL;
	for (int i = 0; i < n; i++)
		TRY(check_stream(c, streams[i]));
	TRY(check_live(c));
	for (int i = 0; i < n; i++)
		mark_restart(c, streams[i]);
	return TFREC_AMD_OK;
}

int tfrec_amd_configure_streams(tfrec_amd_ctx *c, const int32_t *streams, const tfrec_amd_stream_config *cfgs, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !cfgs)))
		return TFREC_AMD_E_INVAL;
	for (int i = 0; i < n; i++) {
		const tfrec_amd_stream_config &sc = cfgs[i];
		TRY(check_stream(c, streams[i]));
		if (sc.types_mask == 0 || (sc.types_mask & ~c->cfg.types_mask) != 0 || sc.thresh < 0 || sc.filter_type < 0 ||
		    sc.filter_type > 1 || sc.reserved != 0) {
			snprintf(g_err, sizeof(g_err), "bad stream config (types_mask 0x%x of the context's 0x%x, thresh %d, filter_type %d, "
				 "reserved %d)", (unsigned)sc.types_mask, (unsigned)c->cfg.types_mask, (int)sc.thresh, (int)sc.filter_type,
				 (int)sc.reserved);
			return TFREC_AMD_E_INVAL;
		}
	}
	TRY(check_live(c));
	if (n == 0)
		return TFREC_AMD_OK;
	// a configure is a reset with new settings: the stream restarts at the next submit (before the first one that restores
	// nothing but the settings)
	for (int i = 0; i < n; i++) {
		const int s = streams[i];
		c->settings.scfg_api[s] = cfgs[i];
		c->settings.scfg[s] = device_cfg(c, cfgs[i]);
		mark_restart(c, s);
	}
	c->settings.n_auto = 0;
	for (const StreamCfg &d : c->settings.scfg)
		c->settings.n_auto += d.autoth;
	use_per_stream(c);
	return TFREC_AMD_OK;
}

int tfrec_amd_get_stream_config(tfrec_amd_ctx *c, int stream, tfrec_amd_stream_config *out)
{
	if (!c || !out || stream < 0 || stream >= c->cfg.n_streams)
		return TFREC_AMD_E_INVAL;
	*out = c->settings.scfg_api[stream];
	return TFREC_AMD_OK;
}

// The phase step per sample, in 2^-32 turns, of a tune of tune_hz at 1536000 P / Q samples per second:
//   inc = floor((tune_hz * 2^33 * Q + 1536000 P) / (2 * 1536000 P)) mod 2^32
// (DESIGN.md 6d at 1/1, 6e at 10/1, 6g at the input rate).  |tune_hz| < 7680000 and Q <= 1536: the numerator reaches 2^66.4, past
// 64 bits from |tune_hz| Q >= 2^30 on, so it is computed in 128.
static uint32_t phase_inc(int32_t tune_hz, long long p, long long q)
{
	const __int128 num = (__int128)tune_hz * ((__int128)1 << 33) * q + 1536000LL * p, den = 2 * 1536000LL * p;
	__int128 v = num / den;
	if (num % den != 0 && num < 0)
		v--;  // (floor, not C's truncation)
	return (uint32_t)(uint64_t)v;
}

// What the three tunes share, behind their own preconditions: every stream and tune checked (out_of_range(tune_hz) writes the
// message) before anything changes; then the tune's hz / inc of the listed streams, their restart -- a tune is a reset with a new
// tune, exactly as a configure is one with new settings -- and its count of tuned streams.
static int tune_common(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *tune_hz, int n, long long p, long long q,
		       const std::function<bool(int32_t)> &out_of_range, Tune &t)
{
	for (int i = 0; i < n; i++) {
		TRY(check_stream(c, streams[i]));
		if (out_of_range(tune_hz[i]))
			return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	for (int i = 0; i < n; i++) {
		const int s = streams[i];
		t.hz[s] = tune_hz[i];
		t.inc[s] = phase_inc(tune_hz[i], p, q);
		mark_restart(c, s);
	}
	t.n_tuned = 0;
	for (const uint32_t v : t.inc)
		t.n_tuned += v != 0;
	return TFREC_AMD_OK;
}

// |tune_hz| < limit, the message of the base and the wide tune
static bool outside_limit(int32_t tune_hz, int limit)
{
	if (tune_hz > -limit && tune_hz < limit)
		return false;
	snprintf(g_err, sizeof(g_err), "tune_hz %d outside (-%d, %d)", (int)tune_hz, limit, limit);
	return true;
}

int tfrec_amd_tune_streams(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *tune_hz, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !tune_hz)))
		return TFREC_AMD_E_INVAL;
	if (c->input.channel()) {
		snprintf(g_err, sizeof(g_err), "the tunes are defined ahead of process_iq: a channel-rate context has none");
		return TFREC_AMD_E_INVAL;
	}
	TRY(tune_common(c, streams, tune_hz, n, 1, 1, [](int32_t hz) { return outside_limit(hz, kTuneLimit); }, c->tunes.narrow));
	if (n > 0)
		use_per_stream(c);
	return TFREC_AMD_OK;
}

int tfrec_amd_get_stream_tune(tfrec_amd_ctx *c, int stream, int32_t *tune_hz)
{
	if (!c || !tune_hz || stream < 0 || stream >= c->cfg.n_streams)
		return TFREC_AMD_E_INVAL;
	*tune_hz = c->tunes.narrow.hz[stream];
	return TFREC_AMD_OK;
}

// a map is a restart that changes the row the stream's tiles are loaded from -- also when it names the row the stream reads already
int tfrec_amd_map_streams(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *inputs, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !inputs)))
		return TFREC_AMD_E_INVAL;
	for (int i = 0; i < n; i++) {
		TRY(check_stream(c, streams[i]));
		if (inputs[i] < 0 || inputs[i] >= c->cfg.n_streams) {
			snprintf(g_err, sizeof(g_err), "input row %d outside [0, %d)", (int)inputs[i], c->cfg.n_streams);
			return TFREC_AMD_E_INVAL;
		}
	}
	TRY(check_live(c));
	if (n == 0)
		return TFREC_AMD_OK;
	for (int i = 0; i < n; i++) {
		c->tunes.row[streams[i]] = inputs[i];
		mark_restart(c, streams[i]);
	}
	c->tunes.mapped = true;
	if (c->input.map_needs_per_stream())
		use_per_stream(c);
	return TFREC_AMD_OK;
}

int tfrec_amd_get_stream_input(tfrec_amd_ctx *c, int stream, int32_t *input)
{
	if (!c || !input || stream < 0 || stream >= c->cfg.n_streams)
		return TFREC_AMD_E_INVAL;
	*input = c->tunes.row[stream];
	return TFREC_AMD_OK;
}

int tfrec_amd_tune_streams_wide(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *tune_hz, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !tune_hz)))
		return TFREC_AMD_E_INVAL;
	if (c->input.kind != PreStage::kDecim10) {
		snprintf(g_err, sizeof(g_err), "the wide tune acts ahead of the 10:1 stage: the context needs the 15.36 MS/s input flag%s",
			 c->input.kind == PreStage::kResample ? " (the tune ahead of the resampling stage is tfrec_amd_tune_streams_input)" : "");
		return TFREC_AMD_E_INVAL;
	}
	return tune_common(c, streams, tune_hz, n, 10, 1, [](int32_t hz) { return outside_limit(hz, kTuneWideLimit); }, c->tunes.wide);
}

int tfrec_amd_get_stream_tune_wide(tfrec_amd_ctx *c, int stream, int32_t *tune_hz)
{
	if (!c || !tune_hz || stream < 0 || stream >= c->cfg.n_streams)
		return TFREC_AMD_E_INVAL;
	*tune_hz = c->tunes.wide.hz[stream];
	return TFREC_AMD_OK;
}

// The tune at the input rate, ahead of the resampling stage (6g); a 10x context's wide tune under another name
int tfrec_amd_tune_streams_input(tfrec_amd_ctx *c, const int32_t *streams, const int32_t *tune_hz, int n)
{
	if (!c || n < 0 || (n > 0 && (!streams || !tune_hz)))
		return TFREC_AMD_E_INVAL;
	if (c->input.kind == PreStage::kDecim10)
		return tfrec_amd_tune_streams_wide(c, streams, tune_hz, n);
	if (!c->input.input_tune()) {
		snprintf(g_err, sizeof(g_err), "the input-rate tune acts ahead of a resampling or 10:1 stage, and this context has none: "
					       "tfrec_amd_tune_streams tunes its 1.536 MS/s input");
		return TFREC_AMD_E_INVAL;
	}
	const long long p = c->input.rate.p, q = c->input.rate.q;
	if (((c->input.rate_abs * 11585) >> 16) >= 32768) {  // (no accepted rate comes near: 19137 at most)
		snprintf(g_err, sizeof(g_err), "input rate %lld/%lld: the int16 store of a tuned stream could wrap", p, q);
		return TFREC_AMD_E_INVAL;
	}
	const auto outside = [p, q](int32_t hz) {  // |tune_hz| < fs_in / 2, in integers
		if (2 * llabs((long long)hz) * q < 1536000LL * p)
			return false;
		snprintf(g_err, sizeof(g_err), "tune_hz %d outside half the input rate 1536000 * %lld / %lld (|tune_hz| < %lld)", (int)hz, p, q,
			 (1536000LL * p + 2 * q - 1) / (2 * q));
		return true;
	};
	return tune_common(c, streams, tune_hz, n, p, q, outside, c->tunes.wide);
}

int tfrec_amd_get_stream_tune_input(tfrec_amd_ctx *c, int stream, int32_t *tune_hz)
{
	return tfrec_amd_get_stream_tune_wide(c, stream, tune_hz);
}
