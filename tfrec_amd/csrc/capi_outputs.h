// tfrec_amd/csrc/capi_outputs.h -- the side outputs' entry points: included by capi.hip, which lists what is where.
#pragma once

// What the three reads share behind their NULL checks (`how`: what turns the output on) -> the oldest undrained submit's set
static int begin_side_read(const tfrec_amd_ctx *c, const SideLane &l, const char *noun, const char *how, int *set)
{
	if (!l.on) {
		snprintf(g_err, sizeof(g_err), "the %s is off: %s", noun, how);
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->inflight == 0) {
		snprintf(g_err, sizeof(g_err), "no undrained submit: the %s is read before tfrec_amd_drain_events", noun);
		return TFREC_AMD_E_STATE;
	}
	*set = c->head;
	return TFREC_AMD_OK;
}

// What the enable calls share behind the checks of their own arguments: not a second time, a live context, no submit so far
static int begin_side_enable(const tfrec_amd_ctx *c, const SideLane &l, const char *noun)
{
	if (l.on) {
		snprintf(g_err, sizeof(g_err), "the %s is enabled already", noun);
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->submitted) {
		snprintf(g_err, sizeof(g_err), "the %s is enabled before the first submit", noun);
		return TFREC_AMD_E_STATE;
	}
	return TFREC_AMD_OK;
}

int tfrec_amd_read_levels(tfrec_amd_ctx *c, tfrec_amd_level *out, size_t cap, int *n_blocks_out)
{
	if (!c || !out || !n_blocks_out)
		return TFREC_AMD_E_INVAL;
	int set = 0;
	TRY(begin_side_read(c, c->lev.lane, "level meter", "tfrec_amd_create makes it with the level meter's flag", &set));
	const size_t n = (size_t)c->cfg.n_streams * (size_t)c->lev.set_blocks[set];
	if (cap < n) {
		snprintf(g_err, sizeof(g_err), "room for %zu level records, the submit has %zu", cap, n);
		return TFREC_AMD_E_INVAL;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[set]));  // (behind the lane's written[set])
	HIPCHK(hipMemcpy(out, c->lev.d_records[set], n * sizeof(tfrec_amd_level), hipMemcpyDeviceToHost));
	*n_blocks_out = c->lev.set_blocks[set];
	return TFREC_AMD_OK;
}

int tfrec_amd_enable_capture(tfrec_amd_ctx *c, uint32_t max_runs, uint64_t max_samples)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	if (max_runs == 0 || max_samples == 0) {
		snprintf(g_err, sizeof(g_err), "max_runs and max_samples must not be 0");
		return TFREC_AMD_E_INVAL;
	}
	TRY(begin_side_enable(c, c->cap.lane, "recorder"));
	if (max_samples > (uint64_t)SIZE_MAX / sizeof(uint32_t)) {
		snprintf(g_err, sizeof(g_err), "max_samples too large");
		return TFREC_AMD_E_NOMEM;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	EnableGuard<CaptureOut> guard(c, c->cap);
	CaptureOut &o = c->cap;
	const size_t n = (size_t)c->cfg.n_streams;
	// a stream's runs in one submit: all but the first and the last are at least 356 samples long, with a gap between them
	o.stage_cap = (int)((size_t)c->cfg.max_blocks * kBlockDec / 356 + 3);
	TRY(own_device(c, o.d_state, n * sizeof(CaptureState)));
	TRY(own_device(c, o.d_stage, n * (size_t)o.stage_cap * sizeof(CaptureStage)));
	TRY(own_device(c, o.d_cnt, n * sizeof(uint2)));
	TRY(own_device(c, o.d_base, n * sizeof(uint4)));
	std::vector<CaptureState> st(n);
	for (size_t s = 0; s < n; s++)  // every stream starts like its FskState (a configure ahead of the first submit is a restart)
		st[s] = CaptureState{ c->settings.scfg[s].thresh, 0, 0, -(1 << 28) };
	HIPCHK(hipMemcpy(o.d_state, st.data(), n * sizeof(CaptureState), hipMemcpyHostToDevice));
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, o.d_runs[k], (size_t)max_runs * sizeof(tfrec_amd_run)));
		TRY(own_device(c, o.d_pool[k], (size_t)max_samples * sizeof(uint32_t)));
		TRY(own_device(c, o.d_hdr[k], sizeof(CaptureHeader)));
	}
	TRY(make_side_lane(c, o.lane));
	o.max_runs = max_runs;
	o.max_samples = max_samples;
	o.lane.on = guard.ok = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_read_captures(tfrec_amd_ctx *c, tfrec_amd_run *runs, size_t cap_runs, uint32_t *n_runs, int16_t *samples, size_t cap_pairs,
			    uint64_t *n_pairs)
{
	if (!c || !n_runs || !n_pairs || (cap_runs > 0 && !runs) || (cap_pairs > 0 && !samples))
		return TFREC_AMD_E_INVAL;
	int set = 0;
	TRY(begin_side_read(c, c->cap.lane, "recorder", "call tfrec_amd_enable_capture before the first submit", &set));
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[set]));  // (behind the lane's written[set])
	const CaptureOut &o = c->cap;
	CaptureHeader hdr;
	HIPCHK(hipMemcpy(&hdr, o.d_hdr[set], sizeof(hdr), hipMemcpyDeviceToHost));
	const bool overflow = hdr.n_runs > o.max_runs || hdr.n_pairs > o.max_samples;
	// the table as far as the device wrote it, then the prefix of whole runs whose pairs it wrote too
	size_t have = (size_t)std::min<unsigned long long>(hdr.n_runs, o.max_runs);
	std::vector<tfrec_amd_run> &tmp = c->cap.tmp;
	tmp.resize(have);
	if (have)
		HIPCHK(hipMemcpy(tmp.data(), o.d_runs[set], have * sizeof(tfrec_amd_run), hipMemcpyDeviceToHost));
	uint64_t pairs = hdr.n_pairs;
	if (overflow) {
		size_t k = 0;
		pairs = 0;
		while (k < have && tmp[k].pool_offset + tmp[k].n_samples <= o.max_samples) {
			pairs = tmp[k].pool_offset + tmp[k].n_samples;
			k++;
		}
		have = k;
	}
	*n_runs = (uint32_t)std::min<unsigned long long>(hdr.n_runs, 0xffffffffull);
	*n_pairs = hdr.n_pairs;
	if (cap_runs < have || (samples && cap_pairs < pairs)) {
		snprintf(g_err, sizeof(g_err), "room for %zu runs and %zu pairs, the submit delivers %zu and %llu", cap_runs, cap_pairs, have,
			 (unsigned long long)pairs);
		return TFREC_AMD_E_INVAL;
	}
	if (!c->restart.set_origin[set].empty()) {  // start_sample counts from the stream's last restart, as end_sample does
		const std::vector<long long> &org = c->restart.set_origin[set];
		for (size_t i = 0; i < have; i++)
			if (tmp[i].stream < org.size())
				tmp[i].start_sample -= org[tmp[i].stream];
	}
	if (samples && pairs)
		HIPCHK(hipMemcpy(samples, o.d_pool[set], (size_t)pairs * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (have)
		memcpy(runs, tmp.data(), have * sizeof(tfrec_amd_run));
	if (overflow && cap_runs > have)
		memset(&runs[have], 0, sizeof(tfrec_amd_run));
	return overflow ? TFREC_AMD_E_OVERFLOW : TFREC_AMD_OK;
}

int tfrec_amd_enable_spectrum(tfrec_amd_ctx *c, int32_t n_bins, int32_t frames_per_record, int32_t max_rows)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	const bool bins_ok = n_bins == 64 || n_bins == 128 || n_bins == 256 || n_bins == 512 || n_bins == 1024;
	if (!bins_ok || frames_per_record < 1 || frames_per_record > 16384 || max_rows < 1 || max_rows > c->cfg.n_streams) {
		snprintf(g_err, sizeof(g_err),
			 "n_bins is 64, 128, 256, 512 or 1024, frames_per_record within [1, 16384], max_rows within [1, n_streams]");
		return TFREC_AMD_E_INVAL;
	}
	if (c->input.channel()) {
		snprintf(g_err, sizeof(g_err), "the spectrum's bounds assume |x| <= 8192: a channel-rate context has none");
		return TFREC_AMD_E_INVAL;
	}
	TRY(begin_side_enable(c, c->spec.lane, "spectrum"));
	HIPCHK(hipSetDevice(c->cfg.device));
	// the largest submit: floor(max_blocks * 32768 * P / Q) complex samples per row
	const long long n_in = (long long)c->cfg.max_blocks * (TFREC_AMD_BLOCK_BYTES / 2) * c->input.rate.p / c->input.rate.q;
	const long long frames = n_in / n_bins;
	const size_t rows = (size_t)max_rows, n = (size_t)n_bins;
	const size_t records = (size_t)((frames + frames_per_record - 1) / frames_per_record);
	EnableGuard<SpectrumOut> guard(c, c->spec);
	SpectrumOut &o = c->spec;
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, o.d_sum[k], rows * records * n * sizeof(unsigned long long)));
		TRY(own_device(c, o.d_peak[k], rows * records * n * sizeof(unsigned long long)));
		TRY(own_device(c, o.d_nf[k], rows * records * sizeof(uint32_t)));
	}
	TRY(make_side_lane(c, o.lane));
	o.n = n_bins;
	o.g = frames_per_record;
	o.rows = max_rows;
	o.max_records = records;
	o.lane.on = guard.ok = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_read_spectrum(tfrec_amd_ctx *c, int32_t row, uint64_t *sum, uint64_t *peak, size_t cap_records, uint32_t *n_frames,
			    int *n_records)
{
	if (!c || !n_records)
		return TFREC_AMD_E_INVAL;
	int set = 0;
	TRY(begin_side_read(c, c->spec.lane, "spectrum", "call tfrec_amd_enable_spectrum before the first submit", &set));
	const SpectrumOut &o = c->spec;
	if (row < 0 || row >= o.set_rows[set]) {
		snprintf(g_err, sizeof(g_err), "row %d: the submit's spectrum covers rows [0, %d)", (int)row, o.set_rows[set]);
		return TFREC_AMD_E_INVAL;
	}
	const size_t nr = (size_t)o.set_records[set], n = (size_t)o.n;
	*n_records = (int)nr;
	if (cap_records < nr || (nr > 0 && (!sum || !peak || !n_frames))) {
		snprintf(g_err, sizeof(g_err), "room for %zu spectrum records, the submit has %zu", cap_records, nr);
		return TFREC_AMD_E_INVAL;
	}
	if (nr == 0)
		return TFREC_AMD_OK;
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[set]));  // (behind the lane's written[set])
	const size_t r0 = (size_t)row * o.max_records;
	HIPCHK(hipMemcpy(sum, o.d_sum[set] + r0 * n, nr * n * sizeof(uint64_t), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(peak, o.d_peak[set] + r0 * n, nr * n * sizeof(uint64_t), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(n_frames, o.d_nf[set] + r0, nr * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return TFREC_AMD_OK;
}

int tfrec_amd_enable_occupancy(tfrec_amd_ctx *c, uint32_t ratio, uint32_t rel)
{
	if (!c)
		return TFREC_AMD_E_INVAL;
	if (ratio < 2 || ratio > 4096 || rel < 1 || rel > 4096) {
		snprintf(g_err, sizeof(g_err), "ratio within [2, 4096], rel within [1, 4096]");
		return TFREC_AMD_E_INVAL;
	}
	if (!c->spec.lane.on) {
		snprintf(g_err, sizeof(g_err), "the occupancy detector works on the spectrum: call tfrec_amd_enable_spectrum first");
		return TFREC_AMD_E_INVAL;
	}
	TRY(begin_side_enable(c, c->occ.lane, "occupancy detector"));
	HIPCHK(hipSetDevice(c->cfg.device));
	EnableGuard<OccupancyOut> guard(c, c->occ);  // (the spectrum's members are not its to reset)
	OccupancyOut &o = c->occ;
	const size_t records = (size_t)c->spec.rows * c->spec.max_records;
	for (int k = 0; k < kSets; k++) {
		TRY(own_device(c, o.d_recs[k], records * sizeof(tfrec_amd_occupancy)));
		TRY(own_device(c, o.d_bits[k], records * (size_t)(c->spec.n / 32) * sizeof(uint32_t)));
	}
	o.ratio = ratio;
	o.rel = rel;
	o.lane.on = guard.ok = true;
	return TFREC_AMD_OK;
}

int tfrec_amd_read_occupancy(tfrec_amd_ctx *c, int32_t row, tfrec_amd_occupancy *recs, uint32_t *bitmap, size_t cap_records, int *n_records)
{
	if (!c || !n_records)
		return TFREC_AMD_E_INVAL;
	int set = 0;
	TRY(begin_side_read(c, c->occ.lane, "occupancy detector", "call tfrec_amd_enable_occupancy before the first submit", &set));
	const SpectrumOut &sp = c->spec;
	if (row < 0 || row >= sp.set_rows[set]) {
		snprintf(g_err, sizeof(g_err), "row %d: the submit's spectrum covers rows [0, %d)", (int)row, sp.set_rows[set]);
		return TFREC_AMD_E_INVAL;
	}
	const size_t nr = (size_t)sp.set_records[set], words = (size_t)(sp.n / 32);
	*n_records = (int)nr;
	if (cap_records < nr || (nr > 0 && (!recs || !bitmap))) {
		snprintf(g_err, sizeof(g_err), "room for %zu occupancy records, the submit has %zu", cap_records, nr);
		return TFREC_AMD_E_INVAL;
	}
	if (nr == 0)
		return TFREC_AMD_OK;
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[set]));  // (behind the spectrum lane's written[set], recorded behind the detector's kernel)
	const size_t r0 = (size_t)row * sp.max_records;
	HIPCHK(hipMemcpy(recs, c->occ.d_recs[set] + r0, nr * sizeof(tfrec_amd_occupancy), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(bitmap, c->occ.d_bits[set] + r0 * words, nr * words * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return TFREC_AMD_OK;
}
