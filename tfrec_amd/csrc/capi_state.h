// tfrec_amd/csrc/capi_state.h -- a stream's state blob: its header, the inventory table, save and load: included by
// capi.hip, which lists what is where.
#pragma once

static_assert(sizeof(tfrec_amd_state_header) == 128 && offsetof(tfrec_amd_state_header, input_kind) == 16 &&
		      offsetof(tfrec_amd_state_header, payload_bytes) == 68 && offsetof(tfrec_amd_state_header, samples_since_restart) == 72 &&
		      offsetof(tfrec_amd_state_header, config) == 80 && offsetof(tfrec_amd_state_header, tune_hz) == 96,
	      "the blob header's layout is documented in tfrec_amd.h and restated in tfrec_amd/state.py");
constexpr size_t kStateSigOff = offsetof(tfrec_amd_state_header, input_kind);
constexpr size_t kStateSigBytes = offsetof(tfrec_amd_state_header, payload_bytes) - kStateSigOff;

static uint64_t state_version_hash()
{
	uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a
	for (const char *p = tfrec_amd_version(); *p; p++)
		h = (h ^ (uint8_t)*p) * 0x100000001b3ull;
	return h;
}

// The inventory of 6b as a table: every piece of state a submit leaves for the next one, per stream, from the records launch_resets
// reads (a pointer the context does not have: no entry) -- plus the stream's settings on the device, which a reset rewrites and a
// load must bring along, and the input correction's row state.  The histories are the buffers the NEXT submit reads (input.sel
// flips per submit), so the table is made per call.
static int state_table(const tfrec_amd_ctx *c, StateTable &T)
{
	T = StateTable{};
	uint32_t off = (uint32_t)sizeof(tfrec_amd_state_header);
	bool full = false;
	auto add = [&](void *base, size_t stride, size_t bytes) {
		if (!base || bytes == 0)
			return;
		if (T.n_seg == kStateSegs) {
			full = true;
			return;
		}
		T.seg[T.n_seg++] = { static_cast<uint8_t *>(base), (unsigned long long)stride, (uint32_t)bytes, off };
		off += ((uint32_t)bytes + 15u) & ~15u;
	};
	const InputPath &I = c->input;
	const size_t n = (size_t)c->cfg.n_streams;
	add(I.history_read(I.tail), (size_t)I.tail.bytes, (size_t)I.tail.bytes);
	add(I.history_read(I.pre), (size_t)I.pre.bytes, (size_t)I.pre.bytes);
	for (int a = 0; a < c->launch.n_active; a++)
		add(c->launch.states[a], sizeof(ChainState), sizeof(ChainState));
	if (c->d_tcarry)
		for (int a = 0; a < c->launch.n_active; a++)
			add(c->d_tcarry + (size_t)a * n, sizeof(int32_t), sizeof(int32_t));
	add(c->d_fsk, sizeof(FskState), sizeof(FskState));
	add(c->lev.d_state, sizeof(LevelState), sizeof(LevelState));
	add(c->cap.d_state, sizeof(CaptureState), sizeof(CaptureState));
	add(c->d_whbx, sizeof(WhbExact), sizeof(WhbExact));
	add(c->d_whbcarry, sizeof(int), sizeof(int));
	add(c->d_whbX, sizeof(ChainState), sizeof(ChainState));
	add(c->decin.d_last, sizeof(uint32_t), sizeof(uint32_t));
	add(c->settings.d_scfg, sizeof(StreamCfg), sizeof(StreamCfg));
	const InputCorrection &o = c->fix;  // (an unmapped stream s reads row s: check_state_streams)
	add(o.dc.d_ring, (size_t)o.dc.k * sizeof(int2), (size_t)o.dc.k * sizeof(int2));
	add(o.dc.d_state, sizeof(int2), sizeof(int2));
	add(o.iq.d_ring, (size_t)o.iq.k * sizeof(IqMoments), (size_t)o.iq.k * sizeof(IqMoments));
	add(o.iq.d_state, sizeof(int2), sizeof(int2));
	if (full) {  // (cannot happen: two histories, two entries per slot and eleven more)
		snprintf(g_err, sizeof(g_err), "state inventory of more than %d entries", kStateSegs);
		return TFREC_AMD_E_STATE;
	}
	T.n_streams = c->cfg.n_streams;
	T.blob_bytes = off;
	return TFREC_AMD_OK;
}

// the header of a blob of this context, but for the stream's own fields
static tfrec_amd_state_header state_signature(const tfrec_amd_ctx *c, uint32_t blob_bytes)
{
	tfrec_amd_state_header h;
	memset(&h, 0, sizeof(h));
	const InputPath &I = c->input;
	h.magic = TFREC_AMD_STATE_MAGIC;
	h.format = TFREC_AMD_STATE_FORMAT;
	h.version_hash = state_version_hash();
	h.input_kind = (int32_t)I.kind;
	h.format_in = I.fmt;
	h.format_pre = I.pre_fmt;
	h.rate_p = I.rate.p;
	h.rate_q = I.rate.q;
	h.tail_bytes = I.tail.bytes;
	h.pre_bytes = I.pre.bytes;
	h.types_mask = (uint32_t)c->cfg.types_mask;
	h.flags = c->cfg.flags & (TFREC_AMD_F_SERIAL_CHAINS | TFREC_AMD_F_LEVELS);
	h.recorder = c->cap.lane.on ? 1u : 0u;
	h.dc_windows = c->fix.dc.k;
	h.iq_windows = c->fix.iq.k;
	h.chain_state_bytes = (uint32_t)sizeof(ChainState);
	h.payload_bytes = blob_bytes - (uint32_t)sizeof(h);
	return h;
}

// What a save and a load ask of their list: every index in range and named once, every stream on its own row and alone on it,
// within the input correction's rows (E_INVAL) -- and nothing pending that the next submit would replace the state with (E_STATE)
static int check_state_streams(const tfrec_amd_ctx *c, const int32_t *streams, int n)
{
	std::vector<uint8_t> seen((size_t)c->cfg.n_streams, 0);
	for (int i = 0; i < n; i++) {
		const int32_t s = streams[i];
		TRY(check_stream(c, s));
		if (seen[s]) {
			snprintf(g_err, sizeof(g_err), "stream %d is listed twice", (int)s);
			return TFREC_AMD_E_INVAL;
		}
		seen[s] = 1;
		if (c->fix.on() && s >= c->fix.rows) {
			snprintf(g_err, sizeof(g_err), "stream %d has no row of the input correction (max_rows %d)", (int)s, c->fix.rows);
			return TFREC_AMD_E_INVAL;
		}
	}
	if (c->tunes.mapped)
		for (int t = 0; t < c->cfg.n_streams; t++) {
			const int32_t row = c->tunes.row[t];
			if (row != t && (seen[t] || seen[row])) {
				snprintf(g_err, sizeof(g_err), "stream %d reads row %d: the state of a mapped or shared row is not saved or loaded", t, (int)row);
				return TFREC_AMD_E_INVAL;
			}
		}
	TRY(check_live(c));
	for (int i = 0; i < n; i++) {
		const int32_t s = streams[i];
		const bool row_reset = (c->fix.dc.k && c->fix.dc.reset_marked[s]) || (c->fix.iq.k && c->fix.iq.reset_marked[s]);
		if (c->restart.marked[s] || row_reset) {
			snprintf(g_err, sizeof(g_err), "stream %d has a %s pending: its state is replaced at the next submit", (int)s,
				 c->restart.marked[s] ? "restart" : "row reset");
			return TFREC_AMD_E_STATE;
		}
	}
	return TFREC_AMD_OK;
}

// the staging buffer and the list, at the first save or load
static int make_state_stage(tfrec_amd_ctx *c, uint32_t blob_bytes)
{
	if (c->state.d_blobs)
		return TFREC_AMD_OK;
	EnableGuard<StateStage> guard(c, c->state);
	TRY(own_device(c, c->state.d_blobs, (size_t)c->cfg.n_streams * blob_bytes));
	TRY(own_device(c, c->state.d_list, (size_t)c->cfg.n_streams * sizeof(int32_t)));
	guard.ok = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_stream_state_bytes(tfrec_amd_ctx *c, size_t *bytes)
{
	if (!c || !bytes)
		return TFREC_AMD_E_INVAL;
	StateTable T;
	TRY(state_table(c, T));
	*bytes = T.blob_bytes;
	return TFREC_AMD_OK;
}

int tfrec_amd_save_streams(tfrec_amd_ctx *c, const int32_t *streams, int n, void *blobs, size_t cap_bytes)
{
	if (!c || n < 0 || (n > 0 && (!streams || !blobs)))
		return TFREC_AMD_E_INVAL;
	TRY(check_state_streams(c, streams, n));
	StateTable T;
	TRY(state_table(c, T));
	const size_t total = (size_t)n * T.blob_bytes;
	if (cap_bytes < total) {
		snprintf(g_err, sizeof(g_err), "room for %zu bytes, %d blobs of %u take %zu", cap_bytes, n, (unsigned)T.blob_bytes, total);
		return TFREC_AMD_E_INVAL;
	}
	if (n == 0)
		return TFREC_AMD_OK;
	TRY(tfrec_amd_sync(c));  // every stage of every submit made has ended: the carried state is that behind the last one
	TRY(make_state_stage(c, T.blob_bytes));
	// (on the copy stream: idle like every other; the header's room and the padding behind a segment stay zero)
	HIPCHK(hipMemcpyAsync(c->state.d_list, streams, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->cpy));
	HIPCHK(hipMemsetAsync(c->state.d_blobs, 0, total, c->cpy));
	HIPCHK(launch_stream_state(c->cpy, false, T, c->state.d_list, n, c->state.d_blobs));
	HIPCHK(hipMemcpyAsync(blobs, c->state.d_blobs, total, hipMemcpyDeviceToHost, c->cpy));
	HIPCHK(hipStreamSynchronize(c->cpy));
	tfrec_amd_state_header h = state_signature(c, T.blob_bytes);
	for (int i = 0; i < n; i++) {
		const int32_t s = streams[i];
		h.samples_since_restart = c->sample_base - c->restart.origin[s];
		h.config = c->settings.scfg_api[s];
		h.tune_hz = c->tunes.narrow.hz[s];
		h.tune_wide_hz = c->input.kind == PreStage::kDecim10 ? c->tunes.wide.hz[s] : 0;
		h.tune_input_hz = c->input.input_tune() ? c->tunes.wide.hz[s] : 0;
		memcpy(static_cast<uint8_t *>(blobs) + (size_t)i * T.blob_bytes, &h, sizeof(h));
	}
	return TFREC_AMD_OK;
}

// one blob's header against this context: everything a load refuses, before it touches anything
static int check_state_blob(const tfrec_amd_ctx *c, const tfrec_amd_state_header &h, const tfrec_amd_state_header &want, int i)
{
	const char *why = nullptr;
	if (h.magic != want.magic)
		why = "the magic";
	else if (h.format != want.format)
		why = "the format version";
	else if (h.version_hash != want.version_hash)
		why = "the build (the hash of tfrec_amd_version())";
	else if (memcmp((const uint8_t *)&h + kStateSigOff, (const uint8_t *)&want + kStateSigOff, kStateSigBytes) != 0)
		why = "the signature (input kind, formats, rate, histories, types mask, serial / levels flags, recorder, DC / IQ windows, chain state size)";
	else if (h.payload_bytes != want.payload_bytes)
		why = "the payload size";
	else if (h.samples_since_restart < 0)
		why = "samples_since_restart";
	if (why) {
		snprintf(g_err, sizeof(g_err), "blob %d: %s does not match this context", i, why);
		return TFREC_AMD_E_INVAL;
	}
	const tfrec_amd_stream_config &sc = h.config;
	if (sc.types_mask == 0 || (sc.types_mask & ~c->cfg.types_mask) != 0 || sc.thresh < 0 || sc.filter_type < 0 || sc.filter_type > 1 ||
	    sc.reserved != 0) {
		snprintf(g_err, sizeof(g_err), "blob %d: bad stream config (types_mask 0x%x of the context's 0x%x, thresh %d, filter_type %d)", i,
			 (unsigned)sc.types_mask, (unsigned)c->cfg.types_mask, (int)sc.thresh, (int)sc.filter_type);
		return TFREC_AMD_E_INVAL;
	}
	const InputPath &I = c->input;
	if (I.channel() ? h.tune_hz != 0 : outside_limit(h.tune_hz, kTuneLimit))
		return TFREC_AMD_E_INVAL;
	bool bad = false;
	if (I.kind == PreStage::kDecim10)
		bad = h.tune_input_hz != h.tune_wide_hz || outside_limit(h.tune_wide_hz, kTuneWideLimit);
	else if (I.kind == PreStage::kResample)
		bad = h.tune_wide_hz != 0 || 2 * llabs((long long)h.tune_input_hz) * I.rate.q >= 1536000LL * I.rate.p ||
		      (h.tune_input_hz != 0 && ((I.rate_abs * 11585) >> 16) >= 32768);
	else
		bad = h.tune_wide_hz != 0 || h.tune_input_hz != 0;
	if (bad) {
		snprintf(g_err, sizeof(g_err), "blob %d: wide tune %d / input tune %d refused by this context's input", i, (int)h.tune_wide_hz,
			 (int)h.tune_input_hz);
		return TFREC_AMD_E_INVAL;
	}
	return TFREC_AMD_OK;
}

int tfrec_amd_load_streams(tfrec_amd_ctx *c, const int32_t *streams, int n, const void *blobs, size_t bytes)
{
	if (!c || n < 0 || (n > 0 && (!streams || !blobs)))
		return TFREC_AMD_E_INVAL;
	TRY(check_state_streams(c, streams, n));
	StateTable T;
	TRY(state_table(c, T));
	const size_t total = (size_t)n * T.blob_bytes;
	if (bytes < total) {
		snprintf(g_err, sizeof(g_err), "%zu bytes given, %d blobs of %u take %zu", bytes, n, (unsigned)T.blob_bytes, total);
		return TFREC_AMD_E_INVAL;
	}
	const tfrec_amd_state_header want = state_signature(c, T.blob_bytes);
	std::vector<tfrec_amd_state_header> hs((size_t)n);
	for (int i = 0; i < n; i++) {
		memcpy(&hs[i], static_cast<const uint8_t *>(blobs) + (size_t)i * T.blob_bytes, sizeof(hs[i]));
		TRY(check_state_blob(c, hs[i], want, i));
	}
	if (n == 0)
		return TFREC_AMD_OK;
	TRY(tfrec_amd_sync(c));
	TRY(make_state_stage(c, T.blob_bytes));
	{
		PoisonGuard guard(c);  // from here on carried state is written: a failure leaves it undefined
		HIPCHK(hipMemcpyAsync(c->state.d_list, streams, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->cpy));
		HIPCHK(hipMemcpyAsync(c->state.d_blobs, blobs, total, hipMemcpyHostToDevice, c->cpy));
		HIPCHK(launch_stream_state(c->cpy, true, T, c->state.d_list, n, c->state.d_blobs));
		HIPCHK(hipStreamSynchronize(c->cpy));  // (the next submit's front-end stream is not ordered behind the copy stream)
		guard.ok = true;
	}
	// The host's side, as tfrec_amd_configure_streams and the tune calls keep it -- without mark_restart.  The kernels read every
	// stream's own settings from now on if this stream's differ from what the uniform kernels assume.
	const long long p = c->input.rate.p, q = c->input.rate.q;
	bool own = false;
	for (int i = 0; i < n; i++) {
		const int32_t s = streams[i];
		const tfrec_amd_state_header &h = hs[i];
		own = own || memcmp(&h.config, &c->settings.scfg_api[s], sizeof(h.config)) != 0 || h.tune_hz != 0;
		c->settings.scfg_api[s] = h.config;
		c->settings.scfg[s] = device_cfg(c, h.config);  // (== the StreamCfg the payload brought: the signature fixes the slots)
		c->tunes.narrow.hz[s] = h.tune_hz;
		c->tunes.narrow.inc[s] = phase_inc(h.tune_hz, 1, 1);
		c->tunes.wide.hz[s] = h.tune_input_hz;
		c->tunes.wide.inc[s] = c->input.input_tune() ? phase_inc(h.tune_input_hz, p, q) : 0u;
		c->restart.origin[s] = c->sample_base - h.samples_since_restart;
	}
	c->settings.n_auto = 0;
	for (const StreamCfg &d : c->settings.scfg)
		c->settings.n_auto += d.autoth;
	for (Tune *t : { &c->tunes.narrow, &c->tunes.wide }) {
		t->n_tuned = 0;
		for (const uint32_t v : t->inc)
			t->n_tuned += v != 0;
	}
	if (own)
		use_per_stream(c);
	c->restart.any = true;  // the origins are no longer all zero: every submit from now on records the ones it ran with
	return TFREC_AMD_OK;
}
