// tfrec_amd/csrc/capi_dc.h -- the DC blocker's entry points: included by capi.hip, which lists what is where.
#pragma once

constexpr int kDcMaxWindows = 4096;  // tfrec_amd_create_dc: the largest avg_windows

int tfrec_amd_create_dc(const tfrec_amd_config *cfg, int32_t format, int32_t rate_p, int32_t rate_q, int32_t avg_windows, int32_t max_rows,
			tfrec_amd_ctx **out)
{
	if (!cfg || !out)
		return TFREC_AMD_E_INVAL;
	*out = nullptr;
	if (format < TFREC_AMD_FMT_U8 || format > TFREC_AMD_FMT_F32) {
		snprintf(g_err, sizeof(g_err), "unknown input format %d", (int)format);
		return TFREC_AMD_E_INVAL;
	}
	if (cfg->flags & TFREC_AMD_F_INPUT_10X) {
		snprintf(g_err, sizeof(g_err), "no DC blocker ahead of the 10:1 stage: the 15.36 MS/s input flag is refused");
		return TFREC_AMD_E_INVAL;
	}
	if (avg_windows < 1 || avg_windows > kDcMaxWindows || max_rows < 1 || max_rows > cfg->n_streams) {
		snprintf(g_err, sizeof(g_err), "avg_windows within [1, %d], max_rows within [1, n_streams]", kDcMaxWindows);
		return TFREC_AMD_E_INVAL;
	}
	const bool base = rate_p == 1 && rate_q == 1;
	if (!base)
		TRY(tfrec_amd_resample_taps(rate_p, rate_q, nullptr, 0, nullptr));
	// the corrected rows are an S16 input whatever the caller's format: the base rate ingests them, a rate resamples them
	return create_with(cfg, format, rate_p, rate_q, !base, base, out, avg_windows, max_rows);
}

int tfrec_amd_get_dc(tfrec_amd_ctx *c, int32_t *avg_windows, int32_t *max_rows)
{
	if (!c || !avg_windows || !max_rows)
		return TFREC_AMD_E_INVAL;
	*avg_windows = c->dc.on ? c->dc.k : 0;
	*max_rows = c->dc.on ? c->dc.rows : 0;
	return TFREC_AMD_OK;
}

int tfrec_amd_read_dc(tfrec_amd_ctx *c, int32_t row, int16_t *d, size_t cap_windows, int *n_windows)
{
	if (!c || !n_windows)
		return TFREC_AMD_E_INVAL;
	*n_windows = 0;
	if (!c->dc.on) {
		snprintf(g_err, sizeof(g_err), "the context has no DC blocker: tfrec_amd_create_dc makes one");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->inflight == 0) {
		snprintf(g_err, sizeof(g_err), "no undrained submit: the DC estimates are read before tfrec_amd_drain_events");
		return TFREC_AMD_E_STATE;
	}
	const int set = c->head;
	const DcBlock &o = c->dc;
	if (row < 0 || row >= o.set_rows[set]) {
		snprintf(g_err, sizeof(g_err), "row %d: the submit used rows [0, %d)", (int)row, o.set_rows[set]);
		return TFREC_AMD_E_INVAL;
	}
	const size_t nw = (size_t)o.set_windows[set];
	*n_windows = (int)nw;
	if (cap_windows < nw || !d) {
		snprintf(g_err, sizeof(g_err), "room for %zu windows, the submit has %zu", cap_windows, nw);
		return TFREC_AMD_E_INVAL;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[set]));  // (behind every chain of the submit, so behind its front-end stream's kernels)
	HIPCHK(hipMemcpy(d, o.d_d[set] + (size_t)row * o.win_stride, nw * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return TFREC_AMD_OK;
}

int tfrec_amd_reset_dc_rows(tfrec_amd_ctx *c, const int32_t *rows, int n)
{
	if (!c || n < 0 || (n > 0 && !rows))
		return TFREC_AMD_E_INVAL;
	if (!c->dc.on) {
		snprintf(g_err, sizeof(g_err), "the context has no DC blocker: tfrec_amd_create_dc makes one");
		return TFREC_AMD_E_INVAL;
	}
	for (int i = 0; i < n; i++)
		if (rows[i] < 0 || rows[i] >= c->dc.rows) {
			snprintf(g_err, sizeof(g_err), "row %d outside [0, %d)", (int)rows[i], c->dc.rows);
			return TFREC_AMD_E_INVAL;
		}
	TRY(check_live(c));
	for (int i = 0; i < n; i++)
		if (!c->dc.reset_marked[rows[i]]) {
			c->dc.reset_marked[rows[i]] = 1;
			c->dc.reset_pending.push_back(rows[i]);
		}
	return TFREC_AMD_OK;
}
