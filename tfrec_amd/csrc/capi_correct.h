// tfrec_amd/csrc/capi_correct.h -- the input correction's entry points, the DC blocker's and the IQ balancer's (6o):
// included by capi.hip, which lists what is where.
#pragma once

constexpr int kDcMaxWindows = 4096;  // tfrec_amd_create_dc: the largest avg_windows
constexpr int kIqMaxWindows = 4096;  // tfrec_amd_create_iq: the largest iq_windows

int tfrec_amd_create_dc(const tfrec_amd_config *cfg, int32_t format, int32_t rate_p, int32_t rate_q, int32_t avg_windows, int32_t max_rows,
			tfrec_amd_ctx **out)
{
	if (!cfg || !out)
		return TFREC_AMD_E_INVAL;
	*out = nullptr;
	TRY(check_input(cfg, format, rate_p, rate_q, "DC blocker"));
	if (avg_windows < 1 || avg_windows > kDcMaxWindows || max_rows < 1 || max_rows > cfg->n_streams) {
		snprintf(g_err, sizeof(g_err), "avg_windows within [1, %d], max_rows within [1, n_streams]", kDcMaxWindows);
		return TFREC_AMD_E_INVAL;
	}
	// the corrected rows are an S16 input whatever the caller's format: the base rate ingests them, a rate resamples them
	return create_with(cfg, InputSpec{ .fmt = format, .p = rate_p, .q = rate_q, .dc_k = avg_windows, .rows = max_rows }, out);
}

int tfrec_amd_create_iq(const tfrec_amd_config *cfg, int32_t format, int32_t rate_p, int32_t rate_q, int32_t dc_windows, int32_t iq_windows,
			int32_t max_rows, tfrec_amd_ctx **out)
{
	if (!cfg || !out)
		return TFREC_AMD_E_INVAL;
	*out = nullptr;
	TRY(check_input(cfg, format, rate_p, rate_q, "IQ balancer"));
	if (dc_windows < 0 || dc_windows > kDcMaxWindows || iq_windows < 1 || iq_windows > kIqMaxWindows || max_rows < 1 ||
	    max_rows > cfg->n_streams) {
		snprintf(g_err, sizeof(g_err), "dc_windows within [0, %d], iq_windows within [1, %d], max_rows within [1, n_streams]", kDcMaxWindows,
			 kIqMaxWindows);
		return TFREC_AMD_E_INVAL;
	}
	return create_with(cfg, InputSpec{ .fmt = format, .p = rate_p, .q = rate_q, .dc_k = dc_windows, .iq_k = iq_windows, .rows = max_rows },
			   out);
}

int tfrec_amd_get_dc(tfrec_amd_ctx *c, int32_t *avg_windows, int32_t *max_rows)
{
	if (!c || !avg_windows || !max_rows)
		return TFREC_AMD_E_INVAL;
	*avg_windows = c->fix.dc.k;
	*max_rows = c->fix.dc.k ? c->fix.rows : 0;
	return TFREC_AMD_OK;
}

int tfrec_amd_get_iq(tfrec_amd_ctx *c, int32_t *iq_windows, int32_t *max_rows)
{
	if (!c || !iq_windows || !max_rows)
		return TFREC_AMD_E_INVAL;
	*iq_windows = c->fix.iq.k;
	*max_rows = c->fix.iq.k ? c->fix.rows : 0;
	return TFREC_AMD_OK;
}

// The two estimators as the entry points below name them: the record in the context and the words of their error texts
template <class Ring>
struct EstimatorRef {
	Estimator<Ring> InputCorrection::*e;
	const char *abbr, *stage, *ctor;
};
static const EstimatorRef<int2> kDcRef = { &InputCorrection::dc, "DC", "DC blocker", "tfrec_amd_create_dc" };
static const EstimatorRef<IqMoments> kIqRef = { &InputCorrection::iq, "IQ", "IQ balancer", "tfrec_amd_create_iq" };

template <class Ring>
static int check_estimator(const tfrec_amd_ctx *c, const EstimatorRef<Ring> &r)
{
	if ((c->fix.*r.e).k)
		return TFREC_AMD_OK;
	snprintf(g_err, sizeof(g_err), "the context has no %s: %s makes one", r.stage, r.ctor);
	return TFREC_AMD_E_INVAL;
}

// tfrec_amd_read_dc, tfrec_amd_read_iq: row `row` of the oldest undrained submit's table of e
template <class Ring>
static int read_estimates(tfrec_amd_ctx *c, const EstimatorRef<Ring> &r, int32_t row, int16_t *dst, size_t cap_windows, int *n_windows)
{
	if (!c || !n_windows)
		return TFREC_AMD_E_INVAL;
	*n_windows = 0;
	TRY(check_estimator(c, r));
	TRY(check_live(c));
	if (c->inflight == 0) {
		snprintf(g_err, sizeof(g_err), "no undrained submit: the %s estimates are read before tfrec_amd_drain_events", r.abbr);
		return TFREC_AMD_E_STATE;
	}
	const int set = c->head;
	const InputCorrection &o = c->fix;
	if (row < 0 || row >= o.set_rows[set]) {
		snprintf(g_err, sizeof(g_err), "row %d: the submit used rows [0, %d)", (int)row, o.set_rows[set]);
		return TFREC_AMD_E_INVAL;
	}
	const size_t nw = (size_t)o.set_windows[set];
	*n_windows = (int)nw;
	if (cap_windows < nw || !dst) {
		snprintf(g_err, sizeof(g_err), "room for %zu windows, the submit has %zu", cap_windows, nw);
		return TFREC_AMD_E_INVAL;
	}
	HIPCHK(hipSetDevice(c->cfg.device));
	HIPCHK(hipEventSynchronize(c->copied[set]));  // (behind every chain of the submit, so behind its front-end stream's kernels)
	HIPCHK(hipMemcpy(dst, (o.*r.e).d_table[set] + (size_t)row * o.win_stride, nw * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return TFREC_AMD_OK;
}

// tfrec_amd_reset_dc_rows, tfrec_amd_reset_iq_rows: the rows start again with the next submit (launch_correct_rows)
template <class Ring>
static int mark_reset_rows(tfrec_amd_ctx *c, const EstimatorRef<Ring> &r, const int32_t *rows, int n)
{
	if (!c || n < 0 || (n > 0 && !rows))
		return TFREC_AMD_E_INVAL;
	TRY(check_estimator(c, r));
	for (int i = 0; i < n; i++)
		if (rows[i] < 0 || rows[i] >= c->fix.rows) {
			snprintf(g_err, sizeof(g_err), "row %d outside [0, %d)", (int)rows[i], c->fix.rows);
			return TFREC_AMD_E_INVAL;
		}
	TRY(check_live(c));
	Estimator<Ring> &e = c->fix.*r.e;
	for (int i = 0; i < n; i++)
		if (!e.reset_marked[rows[i]]) {
			e.reset_marked[rows[i]] = 1;
			e.reset_pending.push_back(rows[i]);
		}
	return TFREC_AMD_OK;
}

int tfrec_amd_read_dc(tfrec_amd_ctx *c, int32_t row, int16_t *d, size_t cap_windows, int *n_windows)
{
	return read_estimates(c, kDcRef, row, d, cap_windows, n_windows);
}

int tfrec_amd_read_iq(tfrec_amd_ctx *c, int32_t row, int16_t *tg, size_t cap_windows, int *n_windows)
{
	return read_estimates(c, kIqRef, row, tg, cap_windows, n_windows);
}

int tfrec_amd_reset_dc_rows(tfrec_amd_ctx *c, const int32_t *rows, int n) { return mark_reset_rows(c, kDcRef, rows, n); }

int tfrec_amd_reset_iq_rows(tfrec_amd_ctx *c, const int32_t *rows, int n) { return mark_reset_rows(c, kIqRef, rows, n); }
