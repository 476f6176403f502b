/* tests/ladder_core.c -- the inner loops of tests/ladder_model.py: the biquad passes' speculate-and-repair ladder of
 * tfrec_amd/csrc/biquad.h (K3a, K3b, K3b', K3c) restated serially for ONE chain and ONE submit, beside the true trajectory.
 * Plain C, compiled with gcc -O2 -ffp-contract=off (the biquad must round after every multiply and add).  TEST INFRASTRUCTURE.
 *
 * With -DLADDER_MAIN the file is a stand-alone program that replays a dump written by ladder_model.dump_chain -- the form in
 * which the sanitizers check it (tests/test_biquad_ladder_cpu.py). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
	double dn1, dn2, yn, yn1;
} lm_state;

enum { LM_SEGMENTS, LM_K3B_UNCONV, LM_K3B2_RUN, LM_K3B2_UNCONV, LM_SERIAL, LM_SERIAL_JOINED, LM_SERIAL_TO_END, LM_SERIAL_HOPS,
       LM_K3B_SLOTS, LM_NCENSUS };
enum { LM_CONVERGED = 0x40000000, LM_RAN = 0x20000000 };

/* iir2::step in the reference's association (dsp_stuff.cpp:28-56) */
static double step(lm_state *f, const double c[5], double dn)
{
	const double y1 = f->yn, y2 = f->yn1;
	const double y = ((c[2] * f->dn2 + c[3] * y1) + (c[0] * dn + c[1] * f->dn1)) + c[4] * y2;
	f->yn1 = y1;
	f->yn = y;
	f->dn2 = f->dn1;
	f->dn1 = dn;
	return y;
}

static int same(double a, double b) { return memcmp(&a, &b, 8) == 0; }
static int same_state(const lm_state *a, const lm_state *b)
{
	return same(a->yn, b->yn) && same(a->yn1, b->yn1) && same(a->dn1, b->dn1) && same(a->dn2, b->dn2);
}

/* the chain input of every decimated sample of a submit: fn(I, Q, previous I, previous Q), the sample ahead of the first one
 * given (prevdec: the stream's last sample of the submit before, zero at a stream's start).  int16: the TFA_2 family's fm_dev
 * array holds int16 values */
typedef int (*lm_fm_fn)(int, int, int, int);
void lm_inputs(lm_fm_fn fn, const int16_t *dec, int m, int prev_i, int prev_q, int as_int16, int32_t *x)
{
	for (int g = 0; g < m; g++) {
		const int v = fn(dec[2 * g], dec[2 * g + 1], prev_i, prev_q);
		x[g] = as_int16 ? (int32_t)(int16_t)v : v;
		prev_i = dec[2 * g];
		prev_q = dec[2 * g + 1];
	}
}

typedef struct {
	const int32_t *x;
	const double *coef;
	int whb, ck_every;
	const int32_t *vslot, *vg0, *vnv; /* per virtual slot: row slot, first sample, samples */
	int32_t *row;
	uint8_t *rung;
} lm_run;

/* one slot: filter its samples, store the slot whole (zeros behind a window's tail) */
static void run_slot(const lm_run *r, lm_state *f, int v, int rung)
{
	int32_t *o = r->row + (size_t)r->vslot[v] * 32;
	for (int k = 0; k < 32; k++) {
		if (k < r->vnv[v]) {
			const int y = (int)step(f, r->coef, (double)r->x[r->vg0[v] + k]);
			o[k] = r->whb ? y : (int32_t)(int16_t)y;
		} else
			o[k] = 0;
	}
	r->rung[r->vslot[v]] = (uint8_t)rung;
}

static int ck_slot(const lm_run *r, int slot) { return (slot & (r->ck_every - 1)) == r->ck_every - 1; }

/* x[m]: the chain's input per sample.  Windows j < nwin of the submit: first sample og[j], nn[j] samples inside the submit.
 * row, true_row [row_slots * 32], rung [row_slots]: the stored outputs after the ladder, the true trajectory in the same
 * layout, and the pass that wrote each slot last (0 none, 1 K3a, 2 K3b, 3 K3b', 4 K3c); the caller fills them beforehand.
 * -> 0, or -1: a slot outside the row, -2: out of memory, -3: windows out of order. */
int lm_chain(const int32_t *x, int m, int nwin, const int32_t *og, const int32_t *nn, const double coef[5], int whb,
	     int seg_slots, int ck_every, int row_slots, const lm_state *carried, int32_t *row, int32_t *true_row, uint8_t *rung,
	     lm_state *ladder_end, lm_state *true_end, long census[LM_NCENSUS])
{
	memset(census, 0, LM_NCENSUS * sizeof(long));
	*ladder_end = *true_end = *carried;
	int vtotal = 0;
	for (int j = 0; j < nwin; j++) {
		if (og[j] < 0 || nn[j] <= 0 || og[j] + nn[j] > m || (j > 0 && og[j] < og[j - 1] + nn[j - 1]))
			return -3;
		vtotal += (nn[j] + 31) >> 5;
	}
	if (vtotal == 0)
		return 0;
	const int nseg = (vtotal + seg_slots - 1) / seg_slots;
	int32_t *vslot = malloc(sizeof(int32_t) * 4 * (size_t)vtotal);
	lm_state *e1 = malloc(sizeof(lm_state) * 3 * (size_t)nseg);
	int32_t *fix = calloc(2 * (size_t)nseg, sizeof(int32_t));
	double *ck = malloc(sizeof(double) * 2 * (size_t)row_slots);
	int rc = 0;
	if (!vslot || !e1 || !fix || !ck) {
		rc = -2;
		goto out;
	}
	int32_t *vg0 = vslot + vtotal, *vnv = vg0 + vtotal, *vwin = vnv + vtotal;
	lm_state *e2 = e1 + nseg, *e3 = e2 + nseg;
	int32_t *fix2 = fix + nseg;
	memset(ck, 0xff, sizeof(double) * 2 * (size_t)row_slots); /* (a NaN pattern no run produces) */
	for (int j = 0, v = 0; j < nwin; j++) {
		const int slot0 = (og[j] >> 5) + j, nch = (nn[j] + 31) >> 5; /* win_slot0 */
		if (slot0 + nch > row_slots) {
			rc = -1;
			goto out;
		}
		for (int i = 0; i < nch; i++, v++) {
			vslot[v] = slot0 + i;
			vg0[v] = og[j] + 32 * i;
			vnv[v] = nn[j] - 32 * i < 32 ? nn[j] - 32 * i : 32;
			vwin[v] = j;
		}
	}
	lm_run r = { x, coef, whb, ck_every, vslot, vg0, vnv, true_row, rung };
	/* the true trajectory: one run over the in-window samples from the carried state */
	for (int v = 0; v < vtotal; v++)
		run_slot(&r, true_end, v, 0);
	r.row = row;
	census[LM_SEGMENTS] = nseg;
#define SEG_LO(k) ((k) * seg_slots)
#define SEG_N(k) (vtotal - SEG_LO(k) < seg_slots ? vtotal - SEG_LO(k) : seg_slots)
	/* K3a: every segment from a zero state; a checkpoint at every ck_every-th slot (by row slot number) */
	for (int k = 0; k < nseg; k++) {
		lm_state f = { 0, 0, 0, 0 };
		for (int d = 0; d < SEG_N(k); d++) {
			const int v = SEG_LO(k) + d;
			run_slot(&r, &f, v, 1);
			if (ck_slot(&r, vslot[v])) {
				ck[2 * vslot[v]] = f.yn;
				ck[2 * vslot[v] + 1] = f.yn1;
			}
		}
		e1[k] = f;
	}
	/* K3b (pass 2) and K3b' (pass 3): the head of the segment again until it joins a checkpoint bit for bit */
	for (int pass = 2; pass <= 3; pass++)
		for (int k = 0; k < nseg; k++) {
			lm_state f;
			int min_slots = 0;
			if (pass == 2)
				f = k > 0 ? e1[k - 1] : *carried;
			else {
				if (!(k > 0 && !(fix[k - 1] & LM_CONVERGED))) {
					fix2[k] = 0;
					continue;
				}
				f = e2[k - 1];
				min_slots = fix[k] & ~LM_CONVERGED;
				census[LM_K3B2_RUN]++;
			}
			int done = 0, nsamples = 0, conv = 0;
			while (1) {
				const int v = SEG_LO(k) + done;
				run_slot(&r, &f, v, pass);
				nsamples += vnv[v];
				done++;
				conv = ck_slot(&r, vslot[v]) && same(f.yn, ck[2 * vslot[v]]) && same(f.yn1, ck[2 * vslot[v] + 1]) &&
				       nsamples >= 2 && done >= min_slots;
				if (conv || done >= SEG_N(k))
					break;
			}
			if (pass == 2) {
				fix[k] = done | (conv ? LM_CONVERGED : 0);
				census[LM_K3B_SLOTS] += done;
				if (!conv) {
					e2[k] = f;
					census[LM_K3B_UNCONV]++;
				}
			} else {
				fix2[k] = done | (conv ? LM_CONVERGED : 0) | LM_RAN;
				if (!conv) {
					e3[k] = f;
					census[LM_K3B2_UNCONV]++;
				}
			}
		}
	/* K3c: the chain walk with the true state (segment 0: K3b ran it from the carried state, the true one) */
	{
		lm_state f = (fix[0] & LM_CONVERGED) ? e1[0] : e2[0];
		for (int k = 1; k < nseg; k++) {
			const int second = (fix2[k] & LM_RAN) != 0;
			const int fx = second ? fix2[k] : fix[k];
			const lm_state from = second ? e2[k - 1] : e1[k - 1];
			if (same_state(&f, &from)) {
				f = (fx & LM_CONVERGED) ? e1[k] : (second ? e3[k] : e2[k]);
				continue;
			}
			census[LM_SERIAL]++;
			const int min_slots = fx & ~(LM_CONVERGED | LM_RAN);
			int done = 0, nsamples = 0, joined = 0, hopped = 0;
			while (1) {
				const int v = SEG_LO(k) + done;
				if (done > 0 && vwin[v] != vwin[v - 1])
					hopped = 1;
				run_slot(&r, &f, v, 4);
				nsamples += vnv[v];
				done++;
				joined = ck_slot(&r, vslot[v]) && same(f.yn, ck[2 * vslot[v]]) && same(f.yn1, ck[2 * vslot[v] + 1]) &&
					 nsamples >= 2 && done >= min_slots;
				if (joined || done >= SEG_N(k))
					break;
			}
			census[LM_SERIAL_HOPS] += hopped;
			if (joined) {
				f = e1[k];
				census[LM_SERIAL_JOINED]++;
			} else
				census[LM_SERIAL_TO_END]++;
		}
		*ladder_end = f;
	}
out:
	free(vslot);
	free(e1);
	free(fix);
	free(ck);
	return rc;
}

#ifdef LADDER_MAIN
#include <stdio.h>

static int stub_fm(int ar, int aj, int br, int bj) { return ar * br + aj * bj; }

/* ladder_core_main DUMP: header int32 {m, nwin, whb, seg_slots, ck_every, row_slots}, double coef[5], lm_state carried,
 * int32 og[nwin], nn[nwin], x[m]; prints the census and whether the ladder's outputs and end state are the true ones */
int main(int argc, char **argv)
{
	if (argc != 2)
		return 2;
	FILE *fp = fopen(argv[1], "rb");
	if (!fp)
		return 2;
	int32_t h[6];
	double coef[5];
	lm_state carried, lend, tend;
	if (fread(h, 4, 6, fp) != 6 || fread(coef, 8, 5, fp) != 5 || fread(&carried, sizeof(carried), 1, fp) != 1)
		return 2;
	const int m = h[0], nwin = h[1], row_slots = h[5];
	int32_t *og = malloc(4 * (size_t)(nwin + 1)), *nn = malloc(4 * (size_t)(nwin + 1)), *x = malloc(4 * (size_t)m);
	int32_t *row = calloc((size_t)row_slots * 32, 4), *tr = calloc((size_t)row_slots * 32, 4);
	uint8_t *rung = calloc((size_t)row_slots, 1);
	if (fread(og, 4, (size_t)nwin, fp) != (size_t)nwin || fread(nn, 4, (size_t)nwin, fp) != (size_t)nwin ||
	    fread(x, 4, (size_t)m, fp) != (size_t)m)
		return 2;
	fclose(fp);
	long census[LM_NCENSUS];
	const int rc = lm_chain(x, m, nwin, og, nn, coef, h[2], h[3], h[4], row_slots, &carried, row, tr, rung, &lend, &tend, census);
	int exact = rc == 0 && same_state(&lend, &tend);
	for (int s = 0; s < row_slots && exact; s++)
		if (rung[s])
			exact = memcmp(row + (size_t)s * 32, tr + (size_t)s * 32, 128) == 0;
	int16_t dec[8] = { 100, -50, 30, 20, -7, 9, 1, 1 };
	int32_t y[4];
	lm_inputs(stub_fm, dec, 4, 0, 0, 1, y);
	printf("rc %d exact %d census", rc, exact);
	for (int i = 0; i < LM_NCENSUS; i++)
		printf(" %ld", census[i]);
	printf(" inputs %d %d %d %d\n", y[0], y[1], y[2], y[3]);
	free(og); free(nn); free(x); free(row); free(tr); free(rung);
	return exact ? 0 : 1;
}
#endif
