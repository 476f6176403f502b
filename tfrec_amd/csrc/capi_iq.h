// tfrec_amd/csrc/capi_iq.h -- the IQ balancer's entry points: included by capi.hip, which lists what is where.
#pragma once

constexpr int kIqMaxWindows = 4096;  // tfrec_amd_create_iq: the largest iq_windows

int tfrec_amd_create_iq(const tfrec_amd_config *cfg, int32_t format, int32_t rate_p, int32_t rate_q, int32_t dc_windows, int32_t iq_windows,
			int32_t max_rows, tfrec_amd_ctx **out)
{
	if (!cfg || !out)
		return TFREC_AMD_E_INVAL;
	*out = nullptr;
	if (format < TFREC_AMD_FMT_U8 || format > TFREC_AMD_FMT_F32) {
		snprintf(g_err, sizeof(g_err), "unknown input format %d", (int)format);
		return TFREC_AMD_E_INVAL;
	}
	if (cfg->flags & TFREC_AMD_F_INPUT_10X) {
		snprintf(g_err, sizeof(g_err), "no IQ balancer ahead of the 10:1 stage: the 15.36 MS/s input flag is refused");
		return TFREC_AMD_E_INVAL;
	}
	if (dc_windows < 0 || dc_windows > kDcMaxWindows || iq_windows < 1 || iq_windows > kIqMaxWindows || max_rows < 1 ||
	    max_rows > cfg->n_streams) {
		snprintf(g_err, sizeof(g_err), "dc_windows within [0, %d], iq_windows within [1, %d], max_rows within [1, n_streams]", kDcMaxWindows,
			 kIqMaxWindows);
		return TFREC_AMD_E_INVAL;
	}
	const bool base = rate_p == 1 && rate_q == 1;
	if (!base)
		TRY(tfrec_amd_resample_taps(rate_p, rate_q, nullptr, 0, nullptr));
	// the corrected rows are an S16 input whatever the caller's format, as behind the DC blocker
	return create_with(cfg, format, rate_p, rate_q, !base, base, out, dc_windows, max_rows, false, iq_windows);
}

int tfrec_amd_get_iq(tfrec_amd_ctx *c, int32_t *iq_windows, int32_t *max_rows)
{
	if (!c || !iq_windows || !max_rows)
		return TFREC_AMD_E_INVAL;
	*iq_windows = c->iq.on ? c->iq.k : 0;
	*max_rows = c->iq.on ? c->iq.rows : 0;
	return TFREC_AMD_OK;
}

int tfrec_amd_read_iq(tfrec_amd_ctx *c, int32_t row, int16_t *tg, size_t cap_windows, int *n_windows)
{
	if (!c || !n_windows)
		return TFREC_AMD_E_INVAL;
	*n_windows = 0;
	if (!c->iq.on) {
		snprintf(g_err, sizeof(g_err), "the context has no IQ balancer: tfrec_amd_create_iq makes one");
		return TFREC_AMD_E_INVAL;
	}
	TRY(check_live(c));
	if (c->inflight == 0) {
		snprintf(g_err, sizeof(g_err), "no undrained submit: the IQ estimates are read before tfrec_amd_drain_events");
		return TFREC_AMD_E_STATE;
	}
	const int set = c->head;
	const IqBal &o = c->iq;
	if (row < 0 || row >= o.set_rows[set]) {
		snprintf(g_err, sizeof(g_err), "row %d: the submit used rows [0, %d)", (int)row, o.set_rows[set]);
		return TFREC_AMD_E_INVAL;
	}
	const size_t nw = (size_t)o.set_windows[set];
	*n_windows = (int)nw;
	if (cap_windows < nw || !tg) {
		snprintf(g_err, sizeof(g_err), "room for %zu windows, the submit has %zu", cap_windows, nw);
		return TFREC_AMD_E_INVAL;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[set]));  // (behind every chain of the submit, so behind its front-end stream's kernels)
	HIPCHK(hipMemcpy(tg, o.d_tg[set] + (size_t)row * o.win_stride, nw * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return TFREC_AMD_OK;
}

int tfrec_amd_reset_iq_rows(tfrec_amd_ctx *c, const int32_t *rows, int n)
{
	if (!c || n < 0 || (n > 0 && !rows))
		return TFREC_AMD_E_INVAL;
	if (!c->iq.on) {
		snprintf(g_err, sizeof(g_err), "the context has no IQ balancer: tfrec_amd_create_iq makes one");
		return TFREC_AMD_E_INVAL;
	}
	for (int i = 0; i < n; i++)
		if (rows[i] < 0 || rows[i] >= c->iq.rows) {
			snprintf(g_err, sizeof(g_err), "row %d outside [0, %d)", (int)rows[i], c->iq.rows);
			return TFREC_AMD_E_INVAL;
		}
	TRY(check_live(c));
	for (int i = 0; i < n; i++)
		if (!c->iq.reset_marked[rows[i]]) {
			c->iq.reset_marked[rows[i]] = 1;
			c->iq.reset_pending.push_back(rows[i]);
		}
	return TFREC_AMD_OK;
}
