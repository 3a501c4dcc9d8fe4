/*
 * Generic compiled-plan host side: gg_engine_compile_plan resolves a
 * gg_plan_desc (engine_abi.h "generalized pipeline descriptor")
 * against registered device columns; exec_plan runs the generic
 * build/scan-agg/compact kernels (plan.hip) and combines partial
 * group states across segments exactly like the reference's two-stage
 * aggregation (cdbgroup.c:1245 / nodeAgg.c:2130–2142: exact partials,
 * one combine).
 *
 * Also here: gg_engine_table_set_nulls (nullable scan surface) and
 * gg_engine_hash_groupby_i64_n (NULL-aware general group-by,
 * execHHashagg.c:531 NULL-key grouping + nodeAgg.c:413 strict
 * transitions).
 */
#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "engine_internal.h"

namespace gg
{

typedef __int128 i128;

struct PlanResolved
{
	PlanDev dev;		/* device pointers resolved; table ptrs live
				 * in the engine registry */
	struct BJoin
	{
		PlanBuildDev bd;	/* preds/key resolved; bits/hkeys
					 * filled per execute (scratch) */
		int64_t dlen;		/* >0: dense bitmap / index map */
		uint64_t hslots;	/* else: hash set / key->index map */
	};
	std::vector<BJoin> joins;
	/* rows of each column source: [0] driving table, [1+k] the build
	 * table of join k */
	int64_t src_rows[1 + GG_PLAN_MAX_JOINS] = {};
	int64_t scan_rows = 0;
	int64_t pred_bytes_per_row = 0;
	/* hipRTC-specialized kernel (nullptr = interpreted fallback);
	 * compiled lazily on first execute, when the join structures'
	 * shape (bitmap vs hash set) is known */
	std::shared_ptr<void> rtc;
	bool rtc_tried = false;
	/* second-stage specialization: after the first execute the
	 * (small) group set is known exactly — tables are immutable —
	 * and gets baked into a direct-indexed kernel */
	std::shared_ptr<void> rtc_baked;
	bool bake_tried = false;
	/* descriptor aggregates in order, lowered onto the device
	 * accumulator slots dev.aggs[] (plan_dev.h PlanAggDev):
	 * MIN/MAX = encoded value word + non-NULL count, AVG = SUM +
	 * count; the helper counts are shared between aggregates over
	 * the same factor columns */
	struct OutAgg
	{
		int kind;	/* gg_plan_aggkind */
		int slot;	/* value / sum accumulator */
		int cnt;	/* helper count accumulator, or -1 */
	};
	std::vector<OutAgg> outs;
	int out_slots = 0;	/* 16-byte arena slots per result row */
	/* packed pair of group columns (dev.gp.packed): 0 = ranges not yet
	 * resolved, 1 = resolved and within budget, 2 = over budget; the
	 * widths are kept for the refusal's message */
	int gp_state = 0;
	int gp_bits[GG_PLAN_MAX_GROUP_COLS] = {0, 0, 0, 0};
	/* three or four group columns (gg_plan_groups): columns 2 and 3 and the
	 * N-field code's parameters, which gp_state covers as it does the
	 * pair's; has_gn = gn.k.n >= 3.  dev.ngroup stays 2 (the columns held by
	 * dev itself) and dev.gp.packed 0; out_ngroup is G */
	PlanGroupNDev gn = {};
	bool has_gn = false;
	/* ORDER BY / LIMIT (gg_plan_desc.order / limit), the order's entries
	 * resolved onto compacted-row words; the device top-k reads the same
	 * entries (engine_internal.h PlanOrderEnt) */
	PlanOrderEnt ord[GG_PLAN_MAX_ORDER] = {};
	int norder = 0;
	int64_t limit = 0;
	/* gg_plan_desc.est_groups, and the group table's slot count once an
	 * execute has settled it (0 = not yet) */
	int64_t est_groups = 0;
	uint64_t nslots = 0;
	/* general WHERE clauses (gg_plan_where): the scope-0 clauses, scan
	 * clauses first (build-scope clauses live in joins[k].bd.wh);
	 * has_where = the plan has a clause of any scope, where0 = one of
	 * scope 0, which is what the scan kernels are selected by */
	PlanWhereDev wh = {};
	bool has_where = false;
	bool where0 = false;
	/* HAVING (gg_plan_having), its atoms resolved onto compacted-row
	 * words; the device selection and the host filter both evaluate hv */
	PlanHavingDev hv = {};
	bool has_having = false;
	/* COUNT(DISTINCT) (engine_abi.h gg_plan_aggkind): `dev` is then the
	 * INNER plan, whose last group column is the distinct column, and
	 * exec_plan regroups its groups by the descriptor's own group columns.
	 * out_ngroup = the descriptor's ngroup, what everything behind the
	 * regroup decodes keys by (dev.ngroup for every other plan); rg = the
	 * fold's view of the inner rows, rg.dmask the distinct slots (0 = no
	 * DISTINCT aggregate), rg.gp copied from dev.gp once that is resolved */
	int out_ngroup = 0;
	PlanRegroupDev rg = {};
};

static int coltype_width(gg_coltype t)
{
	switch (t)
	{
		case GG_COL_CHAR1:
			return 1;
		case GG_COL_INT32:
			return 4;
		default:
			return 8;
	}
}

static gg_status
resolve_pred(Table *t, const gg_plan_pred *in, PlanPredDev *out)
{
	Table::Col *c = t->find(in->col ? in->col : "");

	if (!c)
		return fail(GG_EINVAL, "plan: no column '%s' in table '%s'",
			    in->col ? in->col : "(null)", t->name.c_str());
	out->col = c->dev;
	out->nulls = (const uint8_t *) c->nulls;
	out->width = coltype_width(c->type);
	out->lo = in->lo;
	out->hi = in->hi;
	return GG_OK;
}

extern "C" size_t
gg_engine_plan_desc_size(void)
{
	return sizeof(gg_plan_desc);
}

/* widths of a packed two-column group code (engine_abi.h
 * gg_plan_desc.group_cols).  The span max - min is taken in uint64, where
 * it cannot overflow; span + 1 values plus the NULL code need
 * bit_length(span + 1) bits, 65 where span + 1 is 2^64 itself. */
extern "C" gg_status
gg_engine_plan_group_bits_n(int n, const int64_t *mn, const int64_t *mx,
			    int *bits)
{
	int total = 0;

	if (n < 1 || n > GG_PLAN_MAX_GROUP_COLS || !mn || !mx || !bits)
		return fail(GG_EINVAL, "plan group bits: %d columns", n);
	for (int g = 0; g < n; g++)
	{
		if (mn[g] > mx[g])	/* no rows */
			bits[g] = 1;
		else
		{
			uint64_t span = (uint64_t) mx[g] - (uint64_t) mn[g];

			bits[g] = span == UINT64_MAX ? 65
				: 64 - __builtin_clzll(span + 1);
		}
		total += bits[g];	/* at most 4 x 65 */
	}
	return total <= 62 ? GG_OK : GG_ENOTSUP;
}

extern "C" gg_status
gg_engine_plan_group_bits(const int64_t mn[2], const int64_t mx[2],
			  int bits[2])
{
	return gg_engine_plan_group_bits_n(2, mn, mx, bits);
}

extern "C" size_t
gg_engine_plan_groups_size(void)
{
	return sizeof(gg_plan_groups);
}

/* the table a column source names (engine_abi.h "column sources"):
 * 0 = the driving table, 1+k = the build table of INNER or LEFT join k, where
 * k < limit (njoins, or the probing join's own index for a probe_src) */
static gg_status
resolve_src(const gg_plan_desc *d, Table *scan, int src, int limit,
	    const char *field, int at, Table **out)
{
	if (src == 0)
	{
		*out = scan;
		return GG_OK;
	}
	if (src < 0 || src > d->njoins)
		return fail(GG_EINVAL, "plan: %s %d names source %d, the plan "
			    "has %d joins", field, at, src, d->njoins);
	if (src > limit)
		return fail(GG_EINVAL, "plan: %s %d names source %d, not an "
			    "earlier join", field, at, src);
	if (d->joins[src - 1].kind == GG_JOIN_ANTI)
		return fail(GG_EINVAL, "plan: %s %d names source %d, an ANTI "
			    "join (no payload)", field, at, src);
	if (!gg_join_builds_map(d->joins[src - 1].kind))
		return fail(GG_EINVAL, "plan: %s %d names source %d, a SEMI "
			    "join (no payload)", field, at, src);
	*out = engine_table(d->joins[src - 1].build.table);
	if (!*out)
		return fail(GG_EINVAL, "plan: bad build table (join %d)",
			    src - 1);
	return GG_OK;
}

extern "C" size_t
gg_engine_plan_where_size(void)
{
	return sizeof(gg_plan_where);
}

static bool atom_compares(int kind)
{
	return kind >= GG_ATOM_LT && kind <= GG_ATOM_NE;
}

/* one side of an atom: the column `name` of source `src`, which in a build
 * scope (bt != nullptr) must be 0 and names the build table itself */
static gg_status
resolve_atom_col(const gg_plan_desc *d, Table *scan, Table *bt, int c, int src,
		 const char *name, Table::Col **out)
{
	Table *t = bt;

	if (bt && src != 0)
		return fail(GG_EINVAL, "plan: where clause %d: a build-scope "
			    "atom names source %d (must be 0)", c, src);
	if (!bt)
		GG_TRY(resolve_src(d, scan, src, d->njoins,
				   "atom src of where clause", c, &t));
	*out = t->find(name ? name : "");
	if (!*out)
		return fail(GG_EINVAL, "plan: where clause %d: no column '%s' in "
			    "table '%s'", c, name ? name : "(null)",
			    t->name.c_str());
	return GG_OK;
}

/* Lower the clauses of one scope (0 = the plan's WHERE, 1+k = join k's build
 * filter) into W, scan clauses (every atom of source 0) first: the split is
 * an implementation matter, the result is the conjunction either way.
 * Adds each distinct (column, source) to `seen`. */
static gg_status
lower_where_scope(const gg_plan_desc *d, const gg_plan_where *w, Table *scan,
		  int scope, PlanWhereDev *W,
		  std::vector<std::pair<const void *, int>> &seen, int64_t *bytes)
{
	Table *bt = scope ? engine_table(d->joins[scope - 1].build.table)
		: nullptr;
	int na = 0;

	std::memset(W, 0, sizeof(*W));
	if (scope && !bt)
		return fail(GG_EINVAL, "plan: bad build table (join %d)",
			    scope - 1);
	for (int pass = 0; pass < 2; pass++)
	{
		for (int c = 0; c < w->nclauses; c++)
		{
			const gg_plan_clause *C = &w->clauses[c];
			bool post = false;

			if (C->scope != scope)
				continue;
			for (int q = 0; q < C->natoms; q++)
				if (C->atoms[q].src != 0 ||
				    (atom_compares(C->atoms[q].kind) &&
				     C->atoms[q].src2 != 0))
					post = true;
			if (scope)
				post = false;	/* src != 0 is refused below */
			if (post != (pass == 1))
				continue;
			for (int q = 0; q < C->natoms; q++)
			{
				const gg_plan_atom *A = &C->atoms[q];
				PlanAtomDev &T = W->atoms[na++];
				Table::Col *ca = nullptr, *cb = nullptr;

				GG_TRY(resolve_atom_col(d, scan, bt, c, A->src, A->col,
							&ca));
				T.kind = A->kind;
				T.col = ca->dev;
				T.nulls = (const uint8_t *) ca->nulls;
				T.width = (int8_t) coltype_width(ca->type);
				T.src = A->src;
				T.lo = A->lo;
				T.hi = A->hi;
				if (atom_compares(A->kind))
				{
					GG_TRY(resolve_atom_col(d, scan, bt, c, A->src2,
								A->col2, &cb));
					if ((ca->type == GG_COL_DEC64_S2) !=
					    (cb->type == GG_COL_DEC64_S2))
						return fail(GG_ENOTSUP, "plan: where "
							    "clause %d compares a scaled "
							    "decimal with an integer "
							    "column (fall back to "
							    "standard_ExecutorRun)", c);
					T.col2 = cb->dev;
					T.nulls2 = (const uint8_t *) cb->nulls;
					T.width2 = (int8_t) coltype_width(cb->type);
					T.src2 = A->src2;
				}
				for (int side = 0; side < (cb ? 2 : 1); side++)
				{
					const void *col = side ? T.col2 : T.col;
					int src = side ? T.src2 : T.src;
					bool dup = false;

					for (auto &s : seen)
						if (s.first == col && s.second == src)
							dup = true;
					if (dup)
						continue;
					seen.push_back({col, src});
					*bytes += side ? T.width2 : T.width;
				}
			}
			W->natoms[W->nclauses++] = (int8_t) C->natoms;
		}
		if (pass == 0)
			W->nscan = W->nclauses;
	}
	return GG_OK;
}

/* the extension's own shape (engine_abi.h gg_plan_where, "Errors") */
static gg_status
check_where(const gg_plan_desc *d, const gg_plan_where *w)
{
	int total = 0;

	if (w->nclauses < 0 || w->nclauses > GG_PLAN_MAX_CLAUSES)
		return fail(GG_ENOTSUP, "plan: %d where clauses (fall back to "
			    "standard_ExecutorRun)", w->nclauses);
	for (int c = 0; c < w->nclauses; c++)
	{
		const gg_plan_clause *C = &w->clauses[c];

		if (C->natoms > GG_PLAN_MAX_ATOMS)
			return fail(GG_ENOTSUP, "plan: where clause %d has %d "
				    "atoms (fall back to standard_ExecutorRun)", c,
				    C->natoms);
		if (C->natoms <= 0)
			return fail(GG_EINVAL, "plan: where clause %d is an empty "
				    "disjunction", c);
		total += C->natoms;
		for (int q = 0; q < C->natoms; q++)
			if (C->atoms[q].kind < GG_ATOM_RANGE ||
			    C->atoms[q].kind > GG_ATOM_NOT_NULL)
				return fail(GG_ENOTSUP, "plan: where clause %d atom "
					    "%d kind %d (fall back to "
					    "standard_ExecutorRun)", c, q,
					    C->atoms[q].kind);
	}
	if (total > GG_PLAN_MAX_WHERE_ATOMS)
		return fail(GG_ENOTSUP, "plan: %d where atoms in all (fall back "
			    "to standard_ExecutorRun)", total);
	for (int c = 0; c < w->nclauses; c++)
	{
		const gg_plan_clause *C = &w->clauses[c];

		if (C->scope < 0 || C->scope > d->njoins)
			return fail(GG_EINVAL, "plan: where clause %d scope %d, "
				    "the plan has %d joins", c, C->scope,
				    d->njoins);
		for (int q = 0; q < C->natoms; q++)
			if (atom_compares(C->atoms[q].kind)
			    ? !C->atoms[q].col2 : C->atoms[q].col2 != nullptr)
				return fail(GG_EINVAL, "plan: where clause %d atom "
					    "%d: col2 %s", c, q,
					    C->atoms[q].col2 ? "on a non-comparison"
					    : "missing on a comparison");
	}
	return GG_OK;
}

extern "C" size_t
gg_engine_plan_having_size(void)
{
	return sizeof(gg_plan_having);
}

/* the HAVING's own shape (engine_abi.h gg_plan_having, "Errors") */
static gg_status
check_having(const gg_plan_desc *d, const gg_plan_having *h)
{
	int total = 0;

	if (h->nclauses < 0 || h->nclauses > GG_PLAN_MAX_HAVING_CLAUSES)
		return fail(GG_ENOTSUP, "plan: %d having clauses (fall back to "
			    "standard_ExecutorRun)", h->nclauses);
	for (int c = 0; c < h->nclauses; c++)
	{
		const gg_plan_having_clause *C = &h->clauses[c];

		if (C->natoms > GG_PLAN_MAX_HAVING_ATOMS)
			return fail(GG_ENOTSUP, "plan: having clause %d has %d "
				    "atoms (fall back to standard_ExecutorRun)", c,
				    C->natoms);
		if (C->natoms <= 0)
			return fail(GG_EINVAL, "plan: having clause %d is an "
				    "empty disjunction", c);
		total += C->natoms;
		for (int q = 0; q < C->natoms; q++)
			if (C->atoms[q].kind < GG_HAVING_RANGE ||
			    C->atoms[q].kind > GG_HAVING_NOT_NULL)
				return fail(GG_ENOTSUP, "plan: having clause %d "
					    "atom %d kind %d (fall back to "
					    "standard_ExecutorRun)", c, q,
					    C->atoms[q].kind);
	}
	if (total > GG_PLAN_MAX_HAVING_TOTAL)
		return fail(GG_ENOTSUP, "plan: %d having atoms in all (fall "
			    "back to standard_ExecutorRun)", total);
	for (int c = 0; c < h->nclauses; c++)
		for (int q = 0; q < h->clauses[c].natoms; q++)
		{
			int a = h->clauses[c].atoms[q].agg;

			if (a < 0 || a >= d->naggs)
				return fail(GG_EINVAL, "plan: having clause %d "
					    "atom %d names aggregate %d, the plan "
					    "has %d", c, q, a, d->naggs);
			if (d->aggs[a].kind == GG_AGG_AVG)
				return fail(GG_ENOTSUP, "plan: having clause %d "
					    "atom %d: an AVG cannot be compared "
					    "(fall back to standard_ExecutorRun)",
					    c, q);
		}
	return GG_OK;
}

static gg_status
plan_compile(const gg_plan_desc *d, const gg_plan_where *w,
	     const gg_plan_having *h, const gg_plan_groups *gs,
	     gg_pipeline *out)
{
	Engine &e = engine();

	if (!e.inited)
		return fail(GG_ESTATE, "engine not initialized");
	if (!d || !out)
		return fail(GG_EINVAL, "null plan args");
	Table *scan = engine_table(d->scan.table);

	if (!scan)
		return fail(GG_EINVAL, "plan: bad driving table handle");
	if (d->scan.npreds < 0 || d->scan.npreds > GG_PLAN_MAX_PREDS ||
	    d->njoins < 0 || d->njoins > GG_PLAN_MAX_JOINS ||
	    d->naggs < 1 || d->naggs > GG_PLAN_MAX_AGGS ||
	    d->ngroup < 0 || d->ngroup > 2 ||
	    d->nfilters < 0 || d->nfilters > GG_PLAN_MAX_FILTERS)
		return fail(GG_ENOTSUP, "plan: shape out of v1 bounds "
			    "(fall back to standard_ExecutorRun)");

	/* group columns 2 and 3 (gg_plan_groups) go with a full descriptor */
	if (gs && (gs->ncols < 0 || gs->ncols > GG_PLAN_MAX_GROUP_COLS - 2))
		return fail(GG_ENOTSUP, "plan: %d further group columns (fall "
			    "back to standard_ExecutorRun)", gs->ncols);
	if (gs && d->ngroup != 2)
		return fail(GG_EINVAL, "plan: further group columns need "
			    "ngroup == 2, not %d", d->ngroup);
	const int ngtotal = d->ngroup + (gs ? gs->ncols : 0);

	if (d->limit < 0 || d->norder < 0 || d->norder > GG_PLAN_MAX_ORDER ||
	    d->est_groups < 0)
		return fail(GG_ENOTSUP, "plan: limit %lld, %d order entries or "
			    "est_groups %lld out of bounds (fall back to "
			    "standard_ExecutorRun)", (long long) d->limit,
			    d->norder, (long long) d->est_groups);

	auto pr = std::make_shared<PlanResolved>();
	PlanResolved *R = pr.get();

	std::memset(&R->dev, 0, sizeof(R->dev));
	R->dev.n = scan->nrows;
	R->scan_rows = scan->nrows;
	R->src_rows[0] = scan->nrows;
	R->dev.npreds = d->scan.npreds;
	for (int i = 0; i < d->scan.npreds; i++)
	{
		gg_status st = resolve_pred(scan, &d->scan.preds[i],
					    &R->dev.preds[i]);

		if (st != GG_OK)
			return st;
		R->pred_bytes_per_row += R->dev.preds[i].width;
	}

	/* pred_bytes_per_row, the algorithmic figure: a driving column
	 * counts at its width wherever it is read, as always; a payload
	 * column (source != 0) counts once per plan however many aggregates
	 * read it, plus 4 bytes per INNER or LEFT join for the row index
	 * (an ANTI join counts as a SEMI join does: its probe key) */
	std::vector<std::pair<const void *, int>> payload_seen;
	auto col_bytes = [&](const void *col, int src, int width) -> int
	{
		if (src == 0)
			return width;
		for (auto &q : payload_seen)
			if (q.first == col && q.second == src)
				return 0;
		payload_seen.push_back({col, src});
		return width;
	};

	R->dev.njoins = d->njoins;
	for (int j = 0; j < d->njoins; j++)
	{
		const gg_plan_join *J = &d->joins[j];
		Table *bt = engine_table(J->build.table);

		if (!bt)
			return fail(GG_EINVAL, "plan: bad build table (join %d)",
				    j);
		if (J->build.npreds < 0 ||
		    J->build.npreds > GG_PLAN_MAX_PREDS)
			return fail(GG_ENOTSUP, "plan: join %d pred count", j);
		if (J->kind < GG_JOIN_SEMI || J->kind > GG_JOIN_ANTI)
			return fail(GG_ENOTSUP, "plan: join %d kind", j);
		/* LEFT is the INNER map, ANTI the SEMI set */
		const bool jmap = gg_join_builds_map(J->kind);

		if (jmap && bt->nrows >= 0xFFFFFFFFll)
			return fail(GG_ENOTSUP, "plan: join %d: INNER build "
				    "side of %lld rows (32-bit row indices)", j,
				    (long long) bt->nrows);
		Table *pt = nullptr;

		GG_TRY(resolve_src(d, scan, J->probe_src, j, "probe_src", j,
				   &pt));
		Table::Col *bk = bt->find(J->build_key ? J->build_key : "");
		Table::Col *pk = pt->find(J->probe_key ? J->probe_key : "");

		if (!bk || !pk)
			return fail(GG_EINVAL,
				    "plan: join %d key column missing", j);
		PlanResolved::BJoin bj{};

		bj.bd.kind = J->kind;
		R->src_rows[1 + j] = bt->nrows;

		bj.bd.key = bk->dev;
		bj.bd.knulls = (const uint8_t *) bk->nulls;
		bj.bd.kw = coltype_width(bk->type);
		bj.bd.n = bt->nrows;
		bj.bd.npreds = J->build.npreds;
		for (int i = 0; i < J->build.npreds; i++)
		{
			gg_status st = resolve_pred(bt, &J->build.preds[i],
						    &bj.bd.preds[i]);

			if (st != GG_OK)
				return st;
		}
		R->joins.push_back(bj);
		R->dev.joins[j].pkey = pk->dev;
		R->dev.joins[j].pnulls = (const uint8_t *) pk->nulls;
		R->dev.joins[j].width = coltype_width(pk->type);
		R->dev.pl.jkind[j] = (int8_t) J->kind;
		R->dev.pl.jpsrc[j] = J->probe_src;
		/* the probe key, plus the gathered 4-byte row index */
		R->pred_bytes_per_row +=
			col_bytes(pk->dev, J->probe_src,
				  R->dev.joins[j].width) +
			(jmap ? 4 : 0);
	}

	R->dev.ngroup = d->ngroup;
	for (int g = 0; g < d->ngroup; g++)
	{
		Table *gt = nullptr;

		GG_TRY(resolve_src(d, scan, d->group_src[g], d->njoins,
				   "group_src", g, &gt));
		Table::Col *c = gt->find(d->group_cols[g]
					 ? d->group_cols[g] : "");

		if (!c)
			return fail(GG_EINVAL, "plan: group column missing");
		R->dev.gcol[g] = c->dev;
		R->dev.gnulls[g] = (const uint8_t *) c->nulls;
		R->dev.gwidth[g] = coltype_width(c->type);
		R->dev.pl.gsrc[g] = d->group_src[g];
		R->pred_bytes_per_row += col_bytes(c->dev, d->group_src[g],
						   R->dev.gwidth[g]);
	}
	for (int g = 0; gs && g < gs->ncols; g++)
	{
		Table *gt = nullptr;

		GG_TRY(resolve_src(d, scan, gs->src[g], d->njoins,
				   "group_src", 2 + g, &gt));
		Table::Col *c = gt->find(gs->cols[g] ? gs->cols[g] : "");

		if (!c)
			return fail(GG_EINVAL, "plan: group column missing");
		R->gn.gcol[g] = c->dev;
		R->gn.gnulls[g] = (const uint8_t *) c->nulls;
		R->gn.gwidth[g] = coltype_width(c->type);
		R->gn.gsrc[g] = gs->src[g];
		R->pred_bytes_per_row += col_bytes(c->dev, gs->src[g],
						   R->gn.gwidth[g]);
	}
	if (gs)
	{
		R->gn.k.n = ngtotal;
		R->has_gn = true;
	}
	/* aggregate filters: every one is validated and resolved, referenced
	 * or not; only the referenced ones (fl.used, set below) are ever
	 * evaluated or counted in pred_bytes_per_row */
	for (int k = 0; k < d->nfilters; k++)
	{
		const gg_plan_filter *F = &d->filters[k];

		if (F->npreds < 0 || F->npreds > GG_PLAN_MAX_FILTER_PREDS)
			return fail(GG_ENOTSUP, "plan: filter %d pred count", k);
		R->dev.fl.npreds[k] = (int8_t) F->npreds;
		for (int i = 0; i < F->npreds; i++)
		{
			Table *ft = nullptr;

			GG_TRY(resolve_src(d, scan, F->src[i], d->njoins,
					   "pred src of filter", k, &ft));
			GG_TRY(resolve_pred(ft, &F->preds[i],
					    &R->dev.fl.preds[k][i]));
			R->dev.fl.psrc[k][i] = F->src[i];
		}
	}

	int nacc = 0;
	std::vector<int> helpers;	/* helper count slots so far */
	/* the one column the DISTINCT aggregates count, and its source */
	Table::Col *dcol = nullptr;
	int dsrc = 0;

	for (int a = 0; a < d->naggs; a++)
	{
		const gg_plan_agg *A = &d->aggs[a];
		PlanAggDev T;

		std::memset(&T, 0, sizeof(T));
		if (A->kind < 0 || A->kind > GG_AGG_COUNT_DISTINCT)
			return fail(GG_ENOTSUP, "plan: agg %d kind", a);
		if (A->filter < 0 || A->filter > d->nfilters)
			return fail(GG_EINVAL, "plan: agg %d names filter %d, "
				    "the plan has %d", a, A->filter - 1,
				    d->nfilters);
		if (A->filter && d->filters[A->filter - 1].npreds == 0)
			return fail(GG_EINVAL, "plan: agg %d references filter "
				    "%d, which has no predicates", a,
				    A->filter - 1);
		if (A->kind == GG_AGG_COUNT_DISTINCT)
		{
			if (A->nfactors != 1)
				return fail(GG_ENOTSUP, "plan: agg %d: COUNT(DISTINCT) "
					    "takes exactly one column, not %d factors "
					    "(fall back to standard_ExecutorRun)", a,
					    A->nfactors);
			if (A->mod[0] != GG_FMOD_ID)
				return fail(GG_ENOTSUP, "plan: agg %d: COUNT(DISTINCT) "
					    "takes a plain column, not factor mod %d "
					    "(fall back to standard_ExecutorRun)", a,
					    A->mod[0]);
			if (gs)
				return fail(GG_ENOTSUP, "plan: agg %d: COUNT(DISTINCT) "
					    "with %d group columns (the inner group "
					    "code would hold a fifth field; fall back "
					    "to standard_ExecutorRun)", a, ngtotal);
			if (d->ngroup == 2)
				return fail(GG_ENOTSUP, "plan: agg %d: COUNT(DISTINCT) "
					    "with two group columns (the inner group "
					    "code holds two fields; fall back to "
					    "standard_ExecutorRun)", a);
		}
		if (A->kind == GG_AGG_COUNT_STAR)
			T.nf = 0;
		else if (A->nfactors < 1 || A->nfactors > 3 ||
			 ((A->kind == GG_AGG_COUNT_COL ||
			   A->kind == GG_AGG_MIN || A->kind == GG_AGG_MAX) &&
			  A->nfactors != 1))
			return fail(GG_ENOTSUP, "plan: agg %d factors", a);
		else
			T.nf = A->nfactors;
		for (int f = 0; f < T.nf; f++)
		{
			Table *at = nullptr;

			GG_TRY(resolve_src(d, scan, A->src[f], d->njoins,
					   "agg src of aggregate", a, &at));
			Table::Col *c = at->find(A->col[f] ? A->col[f] : "");

			if (!c)
				return fail(GG_EINVAL,
					    "plan: agg %d column missing", a);
			if (A->mod[f] < 0 || A->mod[f] > 2)
				return fail(GG_ENOTSUP,
					    "plan: agg %d factor mod", a);
			T.col[f] = c->dev;
			T.nulls[f] = (const uint8_t *) c->nulls;
			T.width[f] = coltype_width(c->type);
			T.mod[f] = A->mod[f];
			R->pred_bytes_per_row += col_bytes(c->dev, A->src[f],
							   T.width[f]);
			if (A->kind == GG_AGG_COUNT_DISTINCT)
			{
				if (dcol && (dcol != c || dsrc != A->src[f]))
					return fail(GG_ENOTSUP, "plan: agg %d: "
						    "COUNT(DISTINCT) over more than one "
						    "column in one plan (fall back to "
						    "standard_ExecutorRun)", a);
				dcol = c;
				dsrc = A->src[f];
			}
		}

		/* lower onto accumulator slots; helper slots re-read the
		 * factors' NULL flags only, so they add nothing to
		 * pred_bytes_per_row */
		auto push = [&](int devkind) -> int
		{
			if (nacc >= GG_PLAN_MAX_AGGS)
				return -1;
			R->dev.aggs[nacc] = T;
			R->dev.aggs[nacc].kind = devkind;
			for (int f = 0; f < T.nf; f++)
				R->dev.pl.asrc[nacc][f] = A->src[f];
			/* a helper count inherits its aggregate's filter */
			R->dev.fl.afilt[nacc] = A->filter;
			return nacc++;
		};
		PlanResolved::OutAgg O{A->kind, -1, -1};

		if (A->kind <= GG_AGG_SUM)
			O.slot = push(A->kind);
		else if (A->kind == GG_AGG_COUNT_DISTINCT)
		{
			/* COUNT(x) per (group key, x) pair, under the aggregate's
			 * filter: non-zero iff the value counts */
			O.slot = push(GG_AGG_COUNT_COL);
			if (O.slot >= 0)
				R->rg.dmask |= 1u << O.slot;
		}
		else
		{
			O.slot = push(A->kind == GG_AGG_MIN ? 3
				      : A->kind == GG_AGG_MAX ? 4 : GG_AGG_SUM);
			for (int h : helpers)
			{
				const PlanAggDev &H = R->dev.aggs[h];
				bool same = H.nf == T.nf &&
					R->dev.fl.afilt[h] == A->filter;

				/* same columns read at the same rows, under
				 * the same filter: a table joined twice is
				 * two sources */
				for (int f = 0; same && f < T.nf; f++)
					same = H.col[f] == T.col[f] &&
						R->dev.pl.asrc[h][f] == A->src[f];
				if (same)
					O.cnt = h;
			}
			if (O.cnt < 0 && O.slot >= 0)
			{
				O.cnt = push(GG_AGG_COUNT_COL);
				helpers.push_back(O.cnt);
			}
		}
		if (O.slot < 0 || (A->kind > GG_AGG_SUM &&
				   A->kind != GG_AGG_COUNT_DISTINCT && O.cnt < 0))
			return fail(GG_ENOTSUP,
				    "plan: aggregates need more than %d "
				    "accumulator slots (MIN/MAX/AVG take two)",
				    GG_PLAN_MAX_AGGS);
		R->outs.push_back(O);
		R->out_slots += A->kind == GG_AGG_AVG ? 2 : 1;
	}
	R->dev.naggs = nacc;
	R->out_ngroup = ngtotal;
	if (dcol)
	{
		/* the inner plan: the distinct column, read once more as the
		 * last group column */
		const int g = R->dev.ngroup++;

		R->dev.gcol[g] = dcol->dev;
		R->dev.gnulls[g] = (const uint8_t *) dcol->nulls;
		R->dev.gwidth[g] = coltype_width(dcol->type);
		R->dev.pl.gsrc[g] = (int8_t) dsrc;
		R->pred_bytes_per_row += col_bytes(dcol->dev, dsrc,
						   R->dev.gwidth[g]);
		R->rg.ngroup = R->dev.ngroup;
		R->rg.naggs = nacc;
		for (int a = 0; a < nacc; a++)
			R->rg.kind[a] = (int8_t) R->dev.aggs[a].kind;
	}
	/* two char1 columns keep the e0 * 512 + e1 code; every other pair
	 * is packed by the columns' ranges, resolved at the first execute */
	R->dev.gp.packed = R->dev.ngroup == 2 && !R->has_gn &&
		!(R->dev.gwidth[0] == 1 && R->dev.gwidth[1] == 1);
	for (int a = 0; a < nacc; a++)
		if (R->dev.fl.afilt[a])
			R->dev.fl.used |= 1 << (R->dev.fl.afilt[a] - 1);
	for (int k = 0; k < d->nfilters; k++)
		if (R->dev.fl.used >> k & 1)
			for (int i = 0; i < R->dev.fl.npreds[k]; i++)
				R->pred_bytes_per_row +=
					col_bytes(R->dev.fl.preds[k][i].col,
						  R->dev.fl.psrc[k][i],
						  R->dev.fl.preds[k][i].width);

	/* the order's entries, onto the words of a compacted row */
	for (int o = 0; o < d->norder; o++)
	{
		const gg_plan_order *O = &d->order[o];
		PlanOrderEnt &E = R->ord[o];

		E.desc = O->desc != 0;
		E.nulls_first = O->nulls_first != 0;
		if (O->what == 0)
		{
			if (O->index < 0 || O->index >= ngtotal)
				return fail(GG_EINVAL, "plan: order entry %d names "
					    "group key %d, the plan has %d", o,
					    O->index, ngtotal);
			E.kind = PL_ORD_KEY;
			E.slot = O->index;
		}
		else if (O->what == 1)
		{
			if (O->index < 0 || O->index >= d->naggs)
				return fail(GG_EINVAL, "plan: order entry %d names "
					    "aggregate %d, the plan has %d", o,
					    O->index, d->naggs);
			const PlanResolved::OutAgg &A = R->outs[O->index];

			if (A.kind == GG_AGG_AVG)
				return fail(GG_ENOTSUP, "plan: order entry %d: an "
					    "AVG cannot be an order key", o);
			E.kind = A.kind == GG_AGG_MIN ? PL_ORD_MIN
				: A.kind == GG_AGG_MAX ? PL_ORD_MAX : PL_ORD_I128;
			E.slot = (int8_t) A.slot;
			E.cnt = (int8_t) (A.cnt < 0 ? 0 : A.cnt);
		}
		else
			return fail(GG_EINVAL, "plan: order entry %d: what = %d",
				    o, O->what);
	}
	R->norder = d->norder;
	R->limit = d->limit;
	R->est_groups = d->est_groups;

	if (w)
	{
		/* each distinct (column, source) of the scope-0 clauses counts
		 * once in pred_bytes_per_row, at its width; the builds' rows
		 * are not part of that figure, with or without clauses */
		std::vector<std::pair<const void *, int>> seen;
		int64_t ignored = 0;

		GG_TRY(check_where(d, w));
		GG_TRY(lower_where_scope(d, w, scan, 0, &R->wh, seen,
					 &R->pred_bytes_per_row));
		R->where0 = R->wh.nclauses > 0;
		for (int j = 0; j < d->njoins; j++)
		{
			seen.clear();
			GG_TRY(lower_where_scope(d, w, scan, 1 + j,
						 &R->joins[j].bd.wh, seen, &ignored));
		}
		R->has_where = true;
	}

	if (h)
	{
		/* the atoms, onto the words of a compacted row: what the
		 * order's entries above read for the same aggregate */
		int na = 0;

		GG_TRY(check_having(d, h));
		R->hv.nclauses = h->nclauses;
		for (int c = 0; c < h->nclauses; c++)
		{
			R->hv.natoms[c] = (int8_t) h->clauses[c].natoms;
			for (int q = 0; q < h->clauses[c].natoms; q++)
			{
				const gg_plan_having_atom *A =
					&h->clauses[c].atoms[q];
				const PlanResolved::OutAgg &O = R->outs[A->agg];
				PlanHavingAtomDev &T = R->hv.atoms[na++];

				T.lo_lo = A->lo_lo;
				T.lo_hi = A->lo_hi;
				T.hi_lo = A->hi_lo;
				T.hi_hi = A->hi_hi;
				T.kind = A->kind;
				T.val = O.kind == GG_AGG_MIN ? PL_HV_MIN
					: O.kind == GG_AGG_MAX ? PL_HV_MAX
					: PL_HV_I128;
				T.slot = (int8_t) O.slot;
				T.cnt = (int8_t) (O.cnt < 0 ? 0 : O.cnt);
			}
		}
		R->has_having = true;
	}

	Pipeline *p = new Pipeline();

	p->desc = gg_pipeline_desc{};
	p->desc.kind = (gg_pipeline_kind) GG_PIPE_PLAN_INTERNAL;
	p->plan = pr;
	e.pipelines.push_back(p);
	*out = (gg_pipeline) (e.pipelines.size() - 1);
	return GG_OK;
}

extern "C" gg_status
gg_engine_compile_plan(const gg_plan_desc *d, gg_pipeline *out)
{
	return plan_compile(d, nullptr, nullptr, nullptr, out);
}

extern "C" gg_status
gg_engine_compile_plan_where(const gg_plan_desc *d, const gg_plan_where *w,
			     gg_pipeline *out)
{
	/* no clauses: gg_engine_compile_plan exactly.  A count outside its
	 * bounds is refused once the descriptor itself has been checked */
	return plan_compile(d, w && w->nclauses != 0 ? w : nullptr, nullptr,
			    nullptr, out);
}

extern "C" gg_status
gg_engine_compile_plan_having(const gg_plan_desc *d, const gg_plan_where *w,
			      const gg_plan_having *h, gg_pipeline *out)
{
	/* no clauses: gg_engine_compile_plan_where exactly */
	return plan_compile(d, w && w->nclauses != 0 ? w : nullptr,
			    h && h->nclauses != 0 ? h : nullptr, nullptr, out);
}

extern "C" gg_status
gg_engine_compile_plan_groups(const gg_plan_desc *d, const gg_plan_where *w,
			      const gg_plan_having *h, const gg_plan_groups *g,
			      gg_pipeline *out)
{
	/* no further columns: gg_engine_compile_plan_having exactly */
	return plan_compile(d, w && w->nclauses != 0 ? w : nullptr,
			    h && h->nclauses != 0 ? h : nullptr,
			    g && g->ncols != 0 ? g : nullptr, out);
}

static uint64_t next_pow2_pl(uint64_t v)
{
	uint64_t p = 1;

	while (p < v)
		p <<= 1;
	return p;
}

/* nslots for the generic group table: supports up to ~nslots/2 groups */
static constexpr uint64_t PL_NSLOTS = 1ull << 18;

/* empty the group table and zero the accumulators; the error word is
 * exec_plan's, which clears it ahead of the join builds */
static gg_status
plan_reset_table(hipStream_t s, const PlanDev &D)
{
	GG_HIP(launch_fill_u64(s, D.tkeys, D.nslots, PL_EMPTY));
	GG_HIP(hipMemsetAsync(D.tvals, 0, D.nslots * (size_t) D.naggs * 16,
			      s));
	return GG_OK;
}

/* scan with the generated kernel k (nullptr = the interpreted kernel),
 * compact the used slots into dout / ctr, wait, and read the kernels'
 * error word.  A running timer tm is stopped right after the scan's
 * launch and booked on the plan_scan_agg stat row. */
static gg_status
plan_scan_compact(Engine &e, Pipeline *p, const PlanResolved *R,
		  const std::shared_ptr<void> &k, Timed *tm,
		  unsigned long long *dout, unsigned long long *ctr,
		  unsigned long long *herr)
{
	const PlanDev &D = R->dev;

	const PlanWhereDev *W = R->where0 ? &R->wh : nullptr;
	const PlanGroupNDev *N = R->has_gn ? &R->gn : nullptr;

	if (k)
		GG_TRY(plan_rtc_launch(e.stream, k, D, pl_grid(D.n), 256, W, N));
	else
		GG_HIP(launch_plan_scan_agg(e.stream, D, W, N));
	if (tm)
		p->stat("plan_scan_agg").add(tm->stop(), R->scan_rows, 0,
					     R->scan_rows *
					     R->pred_bytes_per_row);
	GG_HIP(hipMemsetAsync(ctr, 0, 8, e.stream));
	GG_HIP(launch_plan_compact(e.stream, D.tkeys, D.tvals, D.nslots,
				   D.naggs, dout, ctr, D.nslots));
	GG_HIP(hipStreamSynchronize(e.stream));
	GG_HIP(hipMemcpy(herr, D.err, 8, hipMemcpyDeviceToHost));
	return GG_OK;
}

/* overflow-budget proof for the fire-and-forget
 * LDS tier: interval-bound every aggregate value
 * from cached column min/max (immutable data).
 * All values must be non-negative and
 * bound * rows_per_block must clear 2^61 with a
 * 4x margin (long double keeps int64 exact; the
 * margin absorbs product rounding).  An aggregate
 * filter only removes inputs from a sum of
 * non-negative values, so the whole-column bound
 * holds for a filtered plan as it stands.  NULL
 * extension by a LEFT join does the same and no
 * more (a NULL-extended factor is skipped by the
 * strict transition), so it needs no new
 * arithmetic either.  A general WHERE clause
 * (gg_plan_where) only removes rows, so the
 * bounds stay valid under it as well. */
static bool
plan_fast_tier_provable(Engine &e, const PlanResolved *R)
{
	const PlanDev &D = R->dev;
	long double rows_pb = (long double) D.n /
		(long double) pl_grid(D.n) + 256.0L;

	for (int a = 0; a < D.naggs; a++)
	{
		const PlanAggDev &A = D.aggs[a];
		long double lo = 1.0L, hi = 1.0L;

		/* counts add [1,1]; MIN/MAX words
		 * combine by max over a full u64
		 * word and take no part in the
		 * additive bound; an AVG's sum is
		 * a kind-2 slot like any SUM */
		if (A.kind != 2)
			continue;
		for (int f = 0; f < A.nf; f++)
		{
			long long mn, mx;

			/* over the factor's OWN table: a payload column
			 * is bounded by the min/max of the whole build
			 * column (loose but valid), and is only that long */
			if (engine_col_minmax(e, A.col[f], A.width[f],
					      R->src_rows[D.pl.asrc[a][f]],
					      &mn, &mx) != GG_OK)
				return false;
			long double a0 = (long double) mn;
			long double a1 = (long double) mx;

			if (A.mod[f] == 1)
			{
				long double t0 = 100.0L - a1;
				long double t1 = 100.0L - a0;

				a0 = t0;
				a1 = t1;
			}
			else if (A.mod[f] == 2)
			{
				a0 = 100.0L + a0;
				a1 = 100.0L + a1;
			}
			{
				long double c[4] = {
					lo * a0, lo * a1,
					hi * a0, hi * a1};
				long double nl = c[0],
					nh = c[0];

				for (int q = 1; q < 4; q++)
				{
					if (c[q] < nl)
						nl = c[q];
					if (c[q] > nh)
						nh = c[q];
				}
				lo = nl;
				hi = nh;
			}
		}
		if (lo < 0.0L ||
		    hi * rows_pb >=
		    2305843009213693952.0L) /* 2^61 */
			return false;
	}
	return true;
}

/* Packed pair of group columns: resolve the packing parameters at the
 * plan's first execute, ahead of the hipRTC compile that bakes them.
 * Each column is ranged over its own whole table (a payload column over
 * the whole build column: loose but valid, as in the fast-tier proof);
 * with several segments the ranges are first agreed across them, since
 * every segment's codes meet in exec_plan's combine and must pack alike.
 * Widths, acceptance and refusal come from the AGREED ranges only, so
 * the segments all proceed or all refuse: none may leave on its local
 * ranges while the others wait in a collective. */
static gg_status
plan_group_pack(Engine &e, Pipeline *p, PlanResolved *R)
{
	/* the pair, or the G = 3 or 4 columns of a gg_plan_groups plan, whose
	 * columns 2 and 3 live in R->gn */
	const int G = R->has_gn ? R->gn.k.n : 2;

	if (R->gp_state == 0)
	{
		int nseg = e.cfg.n_segments;
		/* an empty column is the identity of the fold below */
		int64_t mn[GG_PLAN_MAX_GROUP_COLS], mx[GG_PLAN_MAX_GROUP_COLS];

		for (int g = 0; g < G; g++)
		{
			const PlanGroupCol C = plan_group_col(R->dev, R->gn, g);
			int64_t rows = R->src_rows[C.src];
			long long a, b;

			mn[g] = INT64_MAX;
			mx[g] = INT64_MIN;
			if (rows <= 0)
				continue;
			GG_TRY(engine_col_minmax(e, C.col, C.width, rows, &a, &b));
			mn[g] = a;
			mx[g] = b;
		}
		if (nseg > 1)
		{
			if (!comm_ready())
				return fail(GG_ESTATE,
					    "multi-segment plan without comm");
			/* the ranges travel as their two's-complement words, 2 * G
			 * of them in one allgather */
			unsigned long long mine[2 * GG_PLAN_MAX_GROUP_COLS];
			std::vector<unsigned long long> all;

			for (int g = 0; g < G; g++)
			{
				mine[2 * g] = (unsigned long long) mn[g];
				mine[2 * g + 1] = (unsigned long long) mx[g];
			}
			GG_TRY(allgather_host_u64(p, "plan.gprange", mine, 2 * G,
						  all));
			for (int r = 0; r < nseg; r++)
				for (int g = 0; g < G; g++)
				{
					mn[g] = std::min(mn[g], (int64_t)
							 all[2 * G * r + 2 * g]);
					mx[g] = std::max(mx[g], (int64_t)
							 all[2 * G * r + 2 * g + 1]);
				}
		}
		R->gp_state = gg_engine_plan_group_bits_n(G, mn, mx, R->gp_bits)
			== GG_OK ? 1 : 2;
		if (R->has_gn)
		{
			int below = 0;

			/* field G-1 is the least significant */
			for (int g = G - 1; g >= 0; g--)
			{
				R->gn.k.gmin[g] = mn[g] > mx[g] ? 0 : mn[g];
				R->gn.k.shift[g] = R->gp_state == 1 ? below : 0;
				below += R->gp_bits[g];
			}
		}
		else
		{
			for (int g = 0; g < 2; g++)
				R->dev.gp.gmin[g] = mn[g] > mx[g] ? 0 : mn[g];
			R->dev.gp.shift = R->gp_bits[1];
		}
	}
	if (R->gp_state == 2 && R->has_gn)
	{
		std::string w = std::to_string(R->gp_bits[0]);

		for (int g = 1; g < G; g++)
			w += " + " + std::to_string(R->gp_bits[g]);
		return fail(GG_ENOTSUP,
			    "plan: %d-column group key needs %s bits, the packed "
			    "code holds 62 (fall back to standard_ExecutorRun)", G,
			    w.c_str());
	}
	if (R->gp_state == 2)
		return fail(GG_ENOTSUP,
			    "plan: 2-column group key needs %d + %d bits, the "
			    "packed code holds 62 (fall back to "
			    "standard_ExecutorRun)", R->gp_bits[0],
			    R->gp_bits[1]);
	p->stat("path_plan_group_packed").launches++;
	if (R->has_gn)
		p->stat("path_plan_group_packed_n").launches++;
	return GG_OK;
}

/* ---- exec_plan's stages, in the order it runs them.  They share the
 * plan R (R->dev.err is the kernels' error word), the 8-byte device
 * counter ctr, and the compacted result: rows of (code, naggs x (lo, hi)),
 * `dout` on the device and `rows` on the host ---- */

/* u64 words per compacted row */
static int
plan_rowsz(const PlanResolved *R)
{
	return 1 + 2 * R->dev.naggs;
}

/* 1. build the join structures (sizing guard as in the named
 * pipelines: dense iff max(key) <= 8x rows).  SEMI: membership
 * bitmap / hash set.  INNER: key -> build-row-index map, dense
 * uint32 array or a row-index array parallel to the hash keys.
 * ANTI builds the SEMI structure and LEFT the INNER one */
static gg_status
plan_build_joins(Engine &e, Pipeline *p, PlanResolved *R,
		 unsigned long long *ctr)
{
	for (size_t j = 0; j < R->joins.size(); j++)
	{
		PlanResolved::BJoin &B = R->joins[j];
		/* LEFT builds what INNER builds, ANTI what SEMI builds
		 * (launch_plan_build maps the kinds the same way) */
		const bool inner = gg_join_builds_map(B.bd.kind);
		char nm[32], nmi[32];
		Timed tm(e.stream);

		if (B.bd.kw == 8 && !B.dlen && !B.hslots)
		{
			unsigned long long maxk = 0;

			GG_TRY(engine_cached_max_i64(
				e, p, (const int64_t *) B.bd.key, B.bd.n,
				ctr, &maxk));
			if (B.bd.n > 0 && maxk > 0 &&
			    maxk <= (unsigned long long) (8 * B.bd.n + 16))
				B.dlen = (int64_t) maxk + 1;
		}
		if (!B.dlen && !B.hslots)
			B.hslots = next_pow2_pl(2 * (uint64_t) B.bd.n + 2);
		std::snprintf(nm, sizeof(nm), "plan.j%zu", j);
		std::snprintf(nmi, sizeof(nmi), "plan.j%zu.idx", j);
		B.bd.err = R->dev.err;
		B.bd.idx = nullptr;
		if (B.dlen && inner)
		{
			uint32_t *idx = (uint32_t *)
				p->sget(nmi, (size_t) B.dlen * 4);

			if (!idx)
				return fail(GG_ENOMEM, "plan join index");
			/* every entry PL_NOROW = absent */
			GG_HIP(hipMemsetAsync(idx, 0xFF, (size_t) B.dlen * 4,
					      e.stream));
			B.bd.idx = idx;
			B.bd.bits = nullptr;
			B.bd.dlen = B.dlen;
			B.bd.hkeys = nullptr;
			B.bd.hslots = 0;
		}
		else if (B.dlen)
		{
			size_t words = (size_t) (B.dlen / 64 + 2);
			unsigned long long *bits = (unsigned long long *)
				p->sget(nm, words * 8);

			if (!bits)
				return fail(GG_ENOMEM, "plan join bitmap");
			GG_HIP(hipMemsetAsync(bits, 0, words * 8, e.stream));
			B.bd.bits = bits;
			B.bd.dlen = B.dlen;
			B.bd.hkeys = nullptr;
			B.bd.hslots = 0;
		}
		else
		{
			unsigned long long *hk = (unsigned long long *)
				p->sget(nm, B.hslots * 8);

			if (!hk)
				return fail(GG_ENOMEM, "plan join set");
			GG_HIP(hipMemsetAsync(hk, 0, B.hslots * 8, e.stream));
			B.bd.bits = nullptr;
			B.bd.dlen = 0;
			B.bd.hkeys = hk;
			B.bd.hslots = B.hslots;
			if (inner)
			{
				/* read only where a key was installed, so
				 * it needs no initial value */
				B.bd.idx = (uint32_t *)
					p->sget(nmi, B.hslots * 4);
				if (!B.bd.idx)
					return fail(GG_ENOMEM,
						    "plan join index");
			}
		}
		GG_HIP(launch_plan_build(e.stream, B.bd));
		p->stat("plan_build").add(tm.stop(), B.bd.n);
		R->dev.joins[j].bits = B.bd.bits;
		R->dev.joins[j].dlen = B.bd.dlen;
		R->dev.joins[j].hkeys = B.bd.hkeys;
		R->dev.joins[j].hslots = B.bd.hslots;
		R->dev.pl.jidx[j] = B.bd.idx;
		p->stat(inner ? (B.dlen ? "path_plan_join_index_dense"
				 : "path_plan_join_index_hash")
			: (B.dlen ? "path_plan_join_bitmap"
			   : "path_plan_join_hash")).launches++;
		/* beside the structure's row: one count per such join and
		 * execute */
		if (B.bd.kind == GG_JOIN_LEFT)
			p->stat("path_plan_join_left").launches++;
		else if (B.bd.kind == GG_JOIN_ANTI)
			p->stat("path_plan_join_anti").launches++;
	}
	return GG_OK;
}

/* 2. group table + fused scan, 3. compact: leaves the segment's *ng_p groups
 * in *dout_p, on the device.  The first execute compiles the plan's generated
 * kernel; a baked kernel that misses is dropped and the execute redone on the
 * generic one; a table sized from an estimate that fills is regrown */
static gg_status
plan_scan_groups(Engine &e, Pipeline *p, PlanResolved *R,
		 unsigned long long *ctr, unsigned long long **dout_p,
		 unsigned long long *ng_p)
{
	/* the fixed table: what every plan without an estimate gets */
	const uint64_t fixed = R->dev.ngroup == 0 ? 1
		: (R->dev.ngroup == 2 ? 1 << 19 : PL_NSLOTS);
	/* with an estimate (gg_plan_desc.est_groups) the table starts at the
	 * estimate and may grow up to `ceiling` slots; there are never more
	 * groups than driving rows, so a table of 2 * rows slots cannot fill */
	const bool growable = R->est_groups > 0 && R->dev.ngroup > 0;
	const uint64_t rows2 = 2 * (uint64_t) std::max<int64_t>(R->scan_rows, 0);
	const uint64_t ceiling = std::max(fixed, next_pow2_pl(rows2));
	uint64_t nslots = R->nslots;
	int naggs = R->dev.naggs;
	int rowsz = plan_rowsz(R);
	unsigned long long *dout = nullptr;
	unsigned long long ng = 0, herr = 0;

	if (!nslots)
		nslots = !growable ? fixed
			: std::max(fixed, next_pow2_pl(std::min(
				2 * (uint64_t) R->est_groups, rows2)));

	/* the table and the compacted output (cap = nslots rows) for the
	 * current nslots.  A growable table is checked against the free
	 * device memory first, counting what the buffers it replaces give
	 * back, and refused rather than left to a failing allocation */
	auto table_alloc = [&]() -> gg_status
	{
		const size_t kb = nslots * 8, vb = nslots * (size_t) naggs * 16,
			ob = nslots * (size_t) rowsz * 8;

		if (growable && nslots > fixed)
		{
			size_t fr = 0, tot = 0, held = 0, need = 0;
			const char *nm[3] = {"plan.tkeys", "plan.tvals",
					     "plan.out"};
			const size_t want[3] = {kb, vb, ob};

			for (int i = 0; i < 3; i++)
				if (p->ssize(nm[i]) < want[i])
				{
					held += p->ssize(nm[i]);
					need += want[i];
				}
			GG_HIP(hipMemGetInfo(&fr, &tot));
			if (need > fr + held)
				return fail(GG_ENOTSUP,
					    "plan: a group table of %llu slots "
					    "needs %zu bytes with its output, %zu "
					    "are free (fall back to "
					    "standard_ExecutorRun)",
					    (unsigned long long) nslots, need,
					    fr + held);
		}
		unsigned long long *tkeys = (unsigned long long *)
			p->sget("plan.tkeys", kb);
		unsigned long long *tvals = (unsigned long long *)
			p->sget("plan.tvals", vb);

		dout = (unsigned long long *) p->sget("plan.out", ob);
		if (!tkeys || !tvals)
			return fail(GG_ENOMEM, "plan group table");
		if (!dout)
			return fail(GG_ENOMEM, "plan out");
		R->dev.tkeys = tkeys;
		R->dev.tvals = tvals;
		R->dev.nslots = nslots;
		return GG_OK;
	};

	GG_TRY(table_alloc());
	{
		Timed tm(e.stream);

		GG_TRY(plan_reset_table(e.stream, R->dev));
		if (!R->rtc_tried)
		{
			/* specialize now: bitmap-vs-hash join shape is
			 * resolved; NULL presence and widths are baked */
			gg_status rs = plan_rtc_compile(
				R->dev, R->dev.gnulls[0] != nullptr,
				R->dev.gnulls[1] != nullptr, &R->rtc, nullptr, 0,
				false, R->where0 ? &R->wh : nullptr,
				R->has_gn ? &R->gn : nullptr);

			R->rtc_tried = true;
			p->stat(rs == GG_OK ? "path_plan_rtc"
				: "path_plan_interp").launches++;
		}
		GG_TRY(plan_scan_compact(e, p, R,
					 R->rtc_baked ? R->rtc_baked : R->rtc,
					 &tm, dout, ctr, &herr));
	}
	if (herr & PL_ERR_DUP_KEY)
		return fail(GG_ENOTSUP,
			    "plan: INNER/LEFT join build key is not unique among "
			    "the build rows that pass (or is INT64_MIN): "
			    "row-multiplying joins are not implemented "
			    "(fall back to standard_ExecutorRun)");
	if (herr == PL_ERR_BAKE_MISS && R->rtc_baked)
	{
		/* the baked kernel saw a group code outside its baked
		 * set (impossible over immutable tables; defensive) —
		 * drop the baked binary and redo this execute on the
		 * generic kernel */
		R->rtc_baked.reset();
		p->stat("path_plan_bake_miss").launches++;
		GG_HIP(hipMemsetAsync(R->dev.err, 0, 8, e.stream));
		GG_TRY(plan_reset_table(e.stream, R->dev));
		GG_TRY(plan_scan_compact(e, p, R, R->rtc, nullptr, dout, ctr,
					 &herr));
	}
	/* the estimate was too low and the table filled: redo the scan on a
	 * table four times the size, until it fits.  The duplicate-key bit
	 * was dealt with above, so the error word can be cleared whole.  The
	 * attempt that filled the table was slow by construction (every late
	 * row probed all of it, pl_slot): the price of an underestimate */
	while (growable && (herr & PL_ERR_FULL) && nslots < ceiling)
	{
		nslots = std::min(nslots * 4, ceiling);
		p->stat("path_plan_group_grow").launches++;
		GG_TRY(table_alloc());
		GG_HIP(hipMemsetAsync(R->dev.err, 0, 8, e.stream));
		Timed tm(e.stream);

		GG_TRY(plan_reset_table(e.stream, R->dev));
		GG_TRY(plan_scan_compact(e, p, R,
					 R->rtc_baked ? R->rtc_baked : R->rtc,
					 &tm, dout, ctr, &herr));
	}
	if (herr)
		return fail(GG_EINVAL,
			    "plan: group cardinality exceeds %llu "
			    "(generic-path v1 cap)",
			    (unsigned long long) nslots / 2);
	/* tables are immutable: later executes start where this one ended */
	R->nslots = nslots;
	GG_HIP(hipMemcpy(&ng, ctr, 8, hipMemcpyDeviceToHost));
	if (ng > nslots)
		return fail(GG_ESTATE, "plan compact overflow");
	*dout_p = dout;
	*ng_p = ng;
	return GG_OK;
}

/* the whole compacted result, copied to the host */
static gg_status
plan_fetch_rows(const PlanResolved *R, const unsigned long long *dout,
		unsigned long long ng, std::vector<unsigned long long> &rows)
{
	rows.resize((size_t) ng * plan_rowsz(R));
	if (ng)
		GG_HIP(hipMemcpy(rows.data(), dout, rows.size() * 8,
				 hipMemcpyDeviceToHost));
	return GG_OK;
}

/* 4. combine partial states across segments (2-stage agg: exact partials
 * + one combine); `rows` becomes the merged groups, ordered by code */
static gg_status
plan_combine_segments(Engine &e, Pipeline *p, const PlanResolved *R,
		      const unsigned long long *dout,
		      std::vector<unsigned long long> &rows)
{
	const int nseg = e.cfg.n_segments, naggs = R->dev.naggs;
	const int rowsz = plan_rowsz(R);
	unsigned long long ng = rows.size() / rowsz;

	if (!comm_ready())
		return fail(GG_ESTATE,
			    "multi-segment plan without comm");
	/* max group count, then padded allgather of rows */
	std::vector<unsigned long long> cnts;
	uint64_t mx = 0;

	GG_TRY(allgather_host_u64(p, "plan.cntg", &ng, 1, cnts));

	for (int r = 0; r < nseg; r++)
		mx = std::max(mx, (uint64_t) cnts[r]);
	size_t per = (size_t) mx * rowsz;

	if (per)
	{
		unsigned long long *ag = (unsigned long long *)
			p->sget("plan.allg",
				(per + per * (size_t) nseg) * 8);

		if (!ag)
			return fail(GG_ENOMEM, "plan allgather");
		GG_HIP(hipMemsetAsync(ag, 0, per * 8, e.stream));
		if (ng)
			GG_HIP(hipMemcpyAsync(ag, dout,
					      (size_t) ng * rowsz * 8,
					      hipMemcpyDeviceToDevice,
					      e.stream));
		GG_HIP(hipStreamSynchronize(e.stream));
		GG_TRY(comm_allgather_u64(ag, ag + per, per));
		std::vector<unsigned long long> all(per *
						    (size_t) nseg);

		GG_HIP(hipMemcpy(all.data(), ag + per,
				 all.size() * 8,
				 hipMemcpyDeviceToHost));

		std::map<long long,
			 std::vector<i128>> merged;

		for (int r = 0; r < nseg; r++)
			for (uint64_t i = 0; i < cnts[r]; i++)
			{
				const unsigned long long *row =
					&all[per * (size_t) r +
					     i * rowsz];
				auto &acc = merged[(long long)
						   row[0]];

				if (acc.empty())
					acc.assign(naggs, 0);
				for (int a = 0; a < naggs; a++)
				{
					i128 v = ((i128) (int64_t)
						  row[2 + 2 * a] << 64) |
						(i128) row[1 + 2 * a];

					/* encoded MIN/MAX words merge by
					 * unsigned max (0 = no input),
					 * everything else by addition */
					if (R->dev.aggs[a].kind >= 3)
						acc[a] = std::max(acc[a], v);
					else
						acc[a] += v;
				}
			}
		rows.clear();
		for (auto &kv : merged)
		{
			rows.push_back((unsigned long long)
				       kv.first);
			for (int a = 0; a < naggs; a++)
			{
				rows.push_back((unsigned long long)
					       (uint64_t)
					       kv.second[a]);
				rows.push_back((unsigned long long)
					       (uint64_t)
					       (kv.second[a] >> 64));
			}
		}
	}
	return GG_OK;
}

/* How the rows behind the regroup of a COUNT(DISTINCT) plan carry their
 * keys, which is how every row of any other plan does: the outer view of the
 * plan.  An outer code is the raw value of the one group column, or 0, under
 * no pack; R->dev stays the inner plan, which the next execute scans. */
static PlanGroupPackDev
plan_out_pack(const PlanResolved *R)
{
	return R->rg.dmask ? PlanGroupPackDev{} : R->dev.gp;
}

/* the group keys an emitted row's code stands for (a NULL key is
 * GG_PLAN_NULL_KEY) */
static void
plan_keys_of(const PlanResolved *R, long long code,
	     int64_t k[GG_PLAN_MAX_GROUP_COLS])
{
	/* the decoder the device top-k shares (plan_keys.h) */
	plan_keys_of(plan_out_pack(R), R->gn.k, R->out_ngroup, code, k);
}

/* (key0 .. key3) ascending as raw int64: the order of an unordered plan's
 * rows and every order's tie-break.  Keys past the plan's columns are 0 on
 * both sides */
static bool
plan_keys_before(const PlanResolved *R, long long ca, long long cb)
{
	int64_t a[GG_PLAN_MAX_GROUP_COLS], b[GG_PLAN_MAX_GROUP_COLS];

	plan_keys_of(R, ca, a);
	plan_keys_of(R, cb, b);
	for (int g = 0; g < GG_PLAN_MAX_GROUP_COLS - 1; g++)
		if (a[g] != b[g])
			return a[g] < b[g];
	return a[GG_PLAN_MAX_GROUP_COLS - 1] < b[GG_PLAN_MAX_GROUP_COLS - 1];
}

/* the value order entry E reads from a compacted row; false = SQL NULL.
 * Group keys and MIN/MAX are int64, COUNT and SUM signed 128-bit */
static bool
plan_order_val(const PlanResolved *R, const PlanOrderEnt &E,
	       const unsigned long long *row, i128 *v)
{
	if (E.kind == PL_ORD_I128)
	{
		*v = ((i128) (int64_t) row[2 + 2 * E.slot] << 64) |
			(i128) row[1 + 2 * E.slot];
		return true;
	}
	if (E.kind == PL_ORD_KEY)
	{
		int64_t k[GG_PLAN_MAX_GROUP_COLS];

		plan_keys_of(R, (long long) row[0], k);
		*v = k[E.slot];
		return k[E.slot] != GG_PLAN_NULL_KEY;
	}
	/* the order-encoded word, decoded as plan_write_arena decodes it */
	unsigned long long e = E.kind == PL_ORD_MIN ? ~row[1 + 2 * E.slot]
		: row[1 + 2 * E.slot];

	*v = (int64_t) (e ^ 0x8000000000000000ull);
	return row[1 + 2 * E.cnt] != 0;
}

/* THE order of a plan's groups (engine_abi.h gg_plan_order): true iff row a
 * comes before row b.  The entries in turn, a NULL placed by nulls_first
 * whatever the direction, then (key0, key1) ascending as raw int64, which
 * is all there is with no entries.  Distinct groups never compare equal.
 * The device top-k (plan_topk.hip) encodes this same order into its sort
 * keys, and its survivors pass through here once more. */
static bool
plan_order_before(const PlanResolved *R, const unsigned long long *a,
		  const unsigned long long *b)
{
	for (int o = 0; o < R->norder; o++)
	{
		const PlanOrderEnt &E = R->ord[o];
		i128 va = 0, vb = 0;
		bool ha = plan_order_val(R, E, a, &va);
		bool hb = plan_order_val(R, E, b, &vb);

		if (ha != hb)	/* one NULL: it goes first iff nulls_first */
			return (!ha) == (E.nulls_first != 0);
		if (ha && va != vb)
			return (va < vb) != (E.desc != 0);
	}
	return plan_keys_before(R, (long long) a[0], (long long) b[0]);
}

/* 5. order the groups and materialize the arena: by decoded keys, or by
 * the plan's order with its limit applied.  This host path serves every
 * ordered plan the device top-k does not: several segments (it runs after
 * plan_combine_segments; a top-k per segment ahead of the combine would be
 * wrong, because a group's partial states live on several segments and no
 * segment can rank it), limit > GG_PLAN_MAX_LIMIT, an order without a limit
 * and tiny group sets.  After a device top-k, `rows` are its survivors and
 * this is their final pass. */
static gg_status
plan_write_arena(const PlanResolved *R,
		 const std::vector<unsigned long long> &rows, void *arena,
		 size_t bytes, size_t *written)
{
	const int rowsz = plan_rowsz(R);
	size_t ng = rows.size() / rowsz;
	std::vector<size_t> order(ng);

	for (size_t i = 0; i < ng; i++)
		order[i] = i;
	if (R->norder == 0 && R->limit == 0)
		std::sort(order.begin(), order.end(),
			  [&](size_t a, size_t b)
		{
			return plan_keys_before(R, (long long) rows[a * rowsz],
						(long long) rows[b * rowsz]);
		});
	else
	{
		auto before = [&](size_t a, size_t b)
		{
			return plan_order_before(R, &rows[a * rowsz],
						 &rows[b * rowsz]);
		};

		if (R->limit > 0 && (uint64_t) R->limit < ng)
		{
			std::partial_sort(order.begin(),
					  order.begin() + R->limit, order.end(),
					  before);
			ng = (size_t) R->limit;
		}
		else
			std::sort(order.begin(), order.end(), before);
	}

	/* a row carries two keys, or all G of a plan with more */
	const size_t keyb = 8 * (size_t) std::max(2, R->out_ngroup);
	size_t need = 16 + (size_t) ng * (keyb + 16 * (size_t) R->out_slots);

	if (bytes < need)
		return fail(GG_EINVAL, "plan arena too small (%zu < %zu)",
			    bytes, need);
	{
		uint8_t *w = (uint8_t *) arena;
		int64_t ng64 = (int64_t) ng;
		int32_t na32 = R->out_slots, ngc32 = R->out_ngroup;

		std::memcpy(w, &ng64, 8);
		std::memcpy(w + 8, &na32, 4);
		std::memcpy(w + 12, &ngc32, 4);
		w += 16;
		for (size_t oi = 0; oi < ng; oi++)
		{
			size_t i = order[oi];
			int64_t k[GG_PLAN_MAX_GROUP_COLS];

			plan_keys_of(R, (long long) rows[i * rowsz], k);
			std::memcpy(w, k, keyb);
			w += keyb;
			for (const PlanResolved::OutAgg &O : R->outs)
			{
				const unsigned long long *v =
					&rows[i * rowsz + 1 + 2 * O.slot];
				unsigned long long cell[2] = {v[0], v[1]};

				if (O.kind == GG_AGG_MIN || O.kind == GG_AGG_MAX)
				{
					/* decode the order-encoded word; N = 0
					 * is SQL NULL (lo = 0) */
					unsigned long long n =
						rows[i * rowsz + 1 + 2 * O.cnt];
					unsigned long long e =
						O.kind == GG_AGG_MIN ? ~v[0] : v[0];

					cell[0] = n ? e ^ 0x8000000000000000ull
						: 0;
					cell[1] = n;
				}
				std::memcpy(w, cell, 16);
				w += 16;
				if (O.kind == GG_AGG_AVG)
				{
					cell[0] = rows[i * rowsz + 1 + 2 * O.cnt];
					cell[1] = 0;
					std::memcpy(w, cell, 16);
					w += 16;
				}
			}
		}
	}
	*written = need;
	return GG_OK;
}

/* a tile's sort keys must fit the device's LDS (160 KiB per workgroup on
 * gfx950; four order entries take 148 KiB) */
static bool
plan_topk_fits(Engine &e, const PlanResolved *R)
{
	int lds = 0;

	if (hipDeviceGetAttribute(&lds,
				  hipDeviceAttributeMaxSharedMemoryPerBlock,
				  e.cfg.device) != hipSuccess)
		return false;
	return plan_topk_lds_bytes(R->norder) <= (size_t) lds;
}

/* 4'. device top-k (plan_topk.hip): tournament rounds over the compacted
 * rows until one tile is left, then only its first `limit` rows come to the
 * host.  The first round's candidates are all ng rows, or, behind a device
 * HAVING, the n0 row indices of its survivor list src0.  There are more
 * candidates than `limit`, so the last tile's head holds `limit` real rows. */
static gg_status
plan_topk_device(Engine &e, Pipeline *p, const PlanResolved *R,
		 const unsigned long long *dout, unsigned long long ng,
		 std::vector<unsigned long long> &rows,
		 const uint32_t *src0 = nullptr, uint64_t n0 = 0)
{
	const int rowsz = plan_rowsz(R);
	const uint64_t limit = (uint64_t) R->limit;
	PlanTopkDev K;

	std::memset(&K, 0, sizeof(K));
	K.rows = dout;
	K.ng = ng;
	K.rowsz = rowsz;
	K.norder = R->norder;
	K.limit = (int) limit;
	K.ngroup = R->out_ngroup;
	K.gp = plan_out_pack(R);
	K.kn = R->gn.k;
	for (int o = 0; o < R->norder; o++)
		K.ord[o] = R->ord[o];

	/* survivors of a round: its tiles x limit indices; the two buffers
	 * alternate, the first round's output being the largest of each */
	const uint64_t ncand = src0 ? n0 : ng;
	const uint64_t t0 = (ncand + PL_TOPK_TILE - 1) / PL_TOPK_TILE;
	const uint64_t t1 = (t0 * limit + PL_TOPK_TILE - 1) / PL_TOPK_TILE;
	uint32_t *buf[2] = {
		(uint32_t *) p->sget("plan.topk.a", t0 * limit * 4),
		(uint32_t *) p->sget("plan.topk.b", t1 * limit * 4)};
	unsigned long long *head = (unsigned long long *)
		p->sget("plan.topk.out", limit * (size_t) rowsz * 8);

	if (!buf[0] || !buf[1] || !head)
		return fail(GG_ENOMEM, "plan top-k scratch");

	Timed tm(e.stream);
	const uint32_t *src = src0;
	uint64_t n = ncand;
	int rounds = 0;

	for (;;)
	{
		const uint64_t tiles = (n + PL_TOPK_TILE - 1) / PL_TOPK_TILE;
		uint32_t *dst = buf[rounds & 1];

		GG_HIP(launch_plan_topk_round(e.stream, K, src, n, dst));
		rounds++;
		src = dst;
		if (tiles == 1)
			break;
		n = tiles * limit;
	}
	GG_HIP(launch_plan_topk_gather(e.stream, K, src, head));
	{
		double ms = tm.stop();
		/* launches counts the tournament's rounds */
		KernelStatAcc &st = p->stat("plan_topk");

		st.launches += rounds;
		st.total_ms += ms;
		st.rows_in += (int64_t) ncand;
		st.rows_out += (int64_t) limit;
	}
	rows.resize((size_t) limit * rowsz);
	GG_HIP(hipMemcpy(rows.data(), head, rows.size() * 8,
			 hipMemcpyDeviceToHost));
	return GG_OK;
}

/* second-stage bake: with the group set observed (and exact —
 * registered tables are immutable), recompile the RTC kernel
 * with the codes as a constexpr compare chain so later
 * executes of this plan skip key probing entirely.  Gated on a
 * small group count (register/LDS budget) and on the first
 * RTC compile having succeeded. */
static void
plan_bake(Engine &e, Pipeline *p, PlanResolved *R,
	  const std::vector<unsigned long long> &rows)
{
	const int rowsz = plan_rowsz(R);
	const size_t ng = rows.size() / rowsz;
	int bake_max = 8;
	const char *bm = getenv("GG_PLAN_BAKE");

	if (bm && bm[0] == '0')
		bake_max = 0;
	if (!R->bake_tried && R->rtc && R->dev.ngroup > 0 &&
	    ng > 0 && (int64_t) ng <= bake_max)
	{
		std::vector<long long> codes(ng);

		for (size_t i = 0; i < ng; i++)
			codes[i] = (long long) rows[i * rowsz];

		bool fastok = plan_fast_tier_provable(e, R);
		gg_status rs = plan_rtc_compile(
			R->dev, R->dev.gnulls[0] != nullptr,
			R->dev.gnulls[1] != nullptr, &R->rtc_baked,
			codes.data(), (int) ng, fastok,
			R->where0 ? &R->wh : nullptr,
			R->has_gn ? &R->gn : nullptr);

		R->bake_tried = true;
		if (rs == GG_OK)
			p->stat(fastok ? "path_plan_rtc_baked_fast"
				: "path_plan_rtc_baked").launches++;
	}
}

/* 3'. device HAVING (plan_having.hip): the indices of the compacted rows
 * whose group passes, in *idx_p, and their number, the one word read back */
static gg_status
plan_having_device(Engine &e, Pipeline *p, const PlanResolved *R,
		   const unsigned long long *dout, unsigned long long ng,
		   unsigned long long *ctr, uint32_t **idx_p, uint64_t *ns_p)
{
	uint32_t *idx = (uint32_t *) p->sget("plan.having.idx",
					      (size_t) ng * 4);
	unsigned long long ns = 0;

	if (!idx)
		return fail(GG_ENOMEM, "plan having scratch");
	Timed tm(e.stream);

	GG_HIP(hipMemsetAsync(ctr, 0, 8, e.stream));
	GG_HIP(launch_plan_having_select(e.stream, R->hv, dout, ng,
					 plan_rowsz(R), idx, ctr));
	{
		double ms = tm.stop();

		GG_HIP(hipStreamSynchronize(e.stream));
		GG_HIP(hipMemcpy(&ns, ctr, 8, hipMemcpyDeviceToHost));
		p->stat("plan_having").add(ms, (int64_t) ng, (int64_t) ns);
	}
	if (ns > ng)
		return fail(GG_ESTATE, "plan having overflow");
	*idx_p = idx;
	*ns_p = ns;
	return GG_OK;
}

/* the survivors of a device HAVING, all ns of them, copied to the host */
static gg_status
plan_having_fetch(Engine &e, Pipeline *p, const PlanResolved *R,
		  const unsigned long long *dout, unsigned long long ng,
		  const uint32_t *idx, uint64_t ns,
		  std::vector<unsigned long long> &rows)
{
	const int rowsz = plan_rowsz(R);

	rows.resize((size_t) ns * rowsz);
	if (!ns)
		return GG_OK;
	unsigned long long *out = (unsigned long long *)
		p->sget("plan.having.out", rows.size() * 8);

	if (!out)
		return fail(GG_ENOMEM, "plan having scratch");
	GG_HIP(launch_plan_having_gather(e.stream, dout, ng, rowsz, idx, ns,
					 out));
	GG_HIP(hipStreamSynchronize(e.stream));
	GG_HIP(hipMemcpy(rows.data(), out, rows.size() * 8,
			 hipMemcpyDeviceToHost));
	return GG_OK;
}

/* 3''. device regroup of a COUNT(DISTINCT) plan (plan_distinct.hip): folds
 * the ng inner groups in dout, one per (group key, value) pair, into the
 * plan's own groups; on return dout / ng are those, rows of the same size */
static gg_status
plan_regroup_device(Engine &e, Pipeline *p, const PlanResolved *R,
		    unsigned long long *ctr, unsigned long long **dout_p,
		    unsigned long long *ng_p)
{
	const unsigned long long ng_in = *ng_p;
	const int naggs = R->dev.naggs, rowsz = plan_rowsz(R);
	/* there are never more groups than pairs, so a table of 2 * pairs
	 * slots cannot fill; without a group column there is one group */
	const uint64_t nslots = R->out_ngroup == 0 ? 1
		: next_pow2_pl(2 * (uint64_t) ng_in);
	const char *nm[3] = {"plan.rg.tkeys", "plan.rg.tvals", "plan.rg.out"};
	const size_t want[3] = {nslots * 8, nslots * (size_t) naggs * 16,
				nslots * (size_t) rowsz * 8};
	size_t fr = 0, tot = 0, held = 0, need = 0;
	unsigned long long ng = 0, herr = 0;

	/* the check a grown group table gets (plan_scan_groups) */
	for (int i = 0; i < 3; i++)
		if (p->ssize(nm[i]) < want[i])
		{
			held += p->ssize(nm[i]);
			need += want[i];
		}
	GG_HIP(hipMemGetInfo(&fr, &tot));
	if (need > fr + held)
		return fail(GG_ENOTSUP,
			    "plan: a regroup table of %llu slots needs %zu bytes "
			    "with its output, %zu are free (fall back to "
			    "standard_ExecutorRun)", (unsigned long long) nslots,
			    need, fr + held);
	unsigned long long *tkeys = (unsigned long long *)
		p->sget(nm[0], want[0]);
	unsigned long long *tvals = (unsigned long long *)
		p->sget(nm[1], want[1]);
	unsigned long long *out = (unsigned long long *)
		p->sget(nm[2], want[2]);

	if (!tkeys || !tvals || !out)
		return fail(GG_ENOMEM, "plan regroup table");
	{
		Timed tm(e.stream);

		GG_HIP(launch_fill_u64(e.stream, tkeys, nslots, PL_EMPTY));
		GG_HIP(hipMemsetAsync(tvals, 0, want[1], e.stream));
		GG_HIP(launch_plan_regroup(e.stream, R->rg, *dout_p, ng_in,
					   rowsz, tkeys, tvals, nslots,
					   R->dev.err));
		GG_HIP(hipMemsetAsync(ctr, 0, 8, e.stream));
		GG_HIP(launch_plan_compact(e.stream, tkeys, tvals, nslots, naggs,
					   out, ctr, nslots));
		double ms = tm.stop();

		GG_HIP(hipStreamSynchronize(e.stream));
		GG_HIP(hipMemcpy(&herr, R->dev.err, 8, hipMemcpyDeviceToHost));
		GG_HIP(hipMemcpy(&ng, ctr, 8, hipMemcpyDeviceToHost));
		p->stat("plan_regroup").add(ms, (int64_t) ng_in, (int64_t) ng);
	}
	if (herr || ng > nslots)
		return fail(GG_ESTATE, "plan regroup table overflow");
	*dout_p = out;
	*ng_p = ng;
	return GG_OK;
}

gg_status
exec_plan(Pipeline *p, void *arena, size_t bytes, size_t *written)
{
	Engine &e = engine();
	PlanResolved *R = (PlanResolved *) p->plan.get();

	if (!R)
		return fail(GG_ESTATE, "not a compiled plan");
	unsigned long long *ctr = (unsigned long long *) p->sget("ctr", 8);

	if (!ctr)
		return fail(GG_ENOMEM, "plan scratch");

	/* the kernels' error word: the INNER builds report duplicate keys
	 * in it, so it is cleared ahead of them, not just before the scan */
	unsigned long long *derr = (unsigned long long *)
		p->sget("plan.err", 8);

	if (!derr)
		return fail(GG_ENOMEM, "plan scratch");
	R->dev.err = derr;
	GG_HIP(hipMemsetAsync(derr, 0, 8, e.stream));
	if (R->dev.gp.packed || R->has_gn)
		GG_TRY(plan_group_pack(e, p, R));
	R->rg.gp = R->dev.gp;

	unsigned long long *dout = nullptr, ng = 0;
	std::vector<unsigned long long> rows;
	const bool ordered = R->norder > 0 || R->limit > 0;
	bool topk = false;

	if (R->has_where)
		p->stat("path_plan_where").launches++;
	GG_TRY(plan_build_joins(e, p, R, ctr));
	GG_TRY(plan_scan_groups(e, p, R, ctr, &dout, &ng));
	/* COUNT(DISTINCT): dout holds the inner plan's (group key, value)
	 * pairs.  They are regrouped on the device with one segment (a pair
	 * seen on two segments counts once, which only the combine by inner
	 * code knows) and more than the handful of pairs the second-stage bake
	 * wants whole on the host; else on the host, below, which then also
	 * evaluates the HAVING and the order */
	const bool distinct = R->rg.dmask != 0;
	bool dhost = false;

	if (distinct)
	{
		/* read once per execute, like GG_PLAN_TOPK */
		const char *dv = getenv("GG_PLAN_DISTINCT");

		dhost = !(e.cfg.n_segments == 1 && ng > 8 &&
			  !(dv && !strcmp(dv, "host")));
		p->stat(dhost ? "path_plan_distinct_host"
			: "path_plan_distinct_device").launches++;
		if (!dhost)
			GG_TRY(plan_regroup_device(e, p, R, ctr, &dout, &ng));
	}
	/* HAVING on the device: one segment (a group's partial states prove
	 * nothing ahead of the combine) and, as for the top-k, more than the
	 * handful of groups the second-stage bake wants whole on the host */
	bool hvdev = false;
	uint32_t *hidx = nullptr;
	uint64_t ns = ng;	/* candidates of the order: groups, or survivors */

	if (R->has_having)
	{
		/* read once per execute, like GG_PLAN_TOPK */
		const char *hv = getenv("GG_PLAN_HAVING");

		hvdev = e.cfg.n_segments == 1 && ng > 8 && ng < PL_TOPK_PAD &&
			!(hv && !strcmp(hv, "host")) && !dhost;
		p->stat(hvdev ? "path_plan_having_device"
			: "path_plan_having_host").launches++;
		if (hvdev)
			GG_TRY(plan_having_device(e, p, R, dout, ng, ctr, &hidx,
						  &ns));
	}
	if (ordered)
	{
		/* read once per execute, like GG_PLAN_BAKE */
		const char *tk = getenv("GG_PLAN_TOPK");

		/* ng > 8 leaves the small group sets, which the second-stage
		 * bake wants whole on the host, to the host path; so does a
		 * HAVING the host evaluates, whose survivors only it knows */
		topk = e.cfg.n_segments == 1 && R->limit > 0 &&
			R->limit <= GG_PLAN_MAX_LIMIT &&
			ns > (uint64_t) R->limit && ng > 8 &&
			ng < PL_TOPK_PAD && !(tk && !strcmp(tk, "host")) &&
			(hvdev || !R->has_having) && !dhost &&
			plan_topk_fits(e, R);
		p->stat(topk ? "path_plan_topk_device"
			: "path_plan_topk_host").launches++;
	}
	if (topk)
		GG_TRY(plan_topk_device(e, p, R, dout, ng, rows, hidx, ns));
	else if (hvdev)
		GG_TRY(plan_having_fetch(e, p, R, dout, ng, hidx, ns, rows));
	else
		GG_TRY(plan_fetch_rows(R, dout, ng, rows));
	if (e.cfg.n_segments > 1)
		GG_TRY(plan_combine_segments(e, p, R, dout, rows));
	if (dhost)
	{
		/* the host's regroup: the bake first, from the FULL set of
		 * inner groups, then the fold the device runs.  A plan without
		 * a group column yields its one row from no pairs at all */
		std::vector<unsigned long long> outer;
		const int rowsz = plan_rowsz(R);

		plan_bake(e, p, R, rows);
		plan_regroup_rows(R->rg, rows, &outer);
		if (outer.empty() && R->out_ngroup == 0)
			outer.assign(rowsz, 0);
		p->stat("plan_regroup").add(0.0, (int64_t) (rows.size() / rowsz),
					    (int64_t) (outer.size() / rowsz));
		rows.swap(outer);
	}
	if (R->has_having && !hvdev)
	{
		/* the host's HAVING: the bake first, from the FULL group set
		 * (a later baked execute must still find every group), then
		 * the row test the device runs */
		const int rowsz = plan_rowsz(R);
		size_t keep = 0;

		if (!distinct)
			plan_bake(e, p, R, rows);
		for (size_t i = 0; i < rows.size() / rowsz; i++)
			if (plan_having_row(R->hv, &rows[i * rowsz]))
			{
				if (keep != i)
					std::memmove(&rows[keep * rowsz],
						     &rows[i * rowsz],
						     (size_t) rowsz * 8);
				keep++;
			}
		rows.resize(keep * rowsz);
	}
	GG_TRY(plan_write_arena(R, rows, arena, bytes, written));
	/* the bake wants the whole group set: a top-k left only its head, a
	 * device HAVING only its survivors, and the host's HAVING baked above;
	 * behind a regroup the rows are not the scan's groups at all */
	if (!topk && !R->has_having && !distinct)
		plan_bake(e, p, R, rows);
	return GG_OK;
}

/* ---- nullable columns ---- */

extern "C" gg_status
gg_engine_table_set_nulls(gg_table t, const char *col,
			  const uint8_t *host_nulls)
{
	Engine &e = engine();

	if (!e.inited)
		return fail(GG_ESTATE, "engine not initialized");
	Table *tab = engine_table(t);

	if (!tab)
		return fail(GG_EINVAL, "bad table handle");
	Table::Col *c = tab->find(col ? col : "");

	if (!c)
		return fail(GG_EINVAL, "no column '%s'", col ? col : "");
	if (!host_nulls)
		return fail(GG_EINVAL, "null flags pointer");
	if (!c->nulls)
		GG_HIP(hipMalloc(&c->nulls, (size_t) tab->nrows));
	GG_HIP(hipMemcpy(c->nulls, host_nulls, (size_t) tab->nrows,
			 hipMemcpyHostToDevice));
	return GG_OK;
}

/* ---- NULL-aware general hash group-by ----
 * Reuses the in-memory group-by kernels twice: pass A aggregates
 * NULL-mapped keys with NULL vals as 0 (sums exact since strict SUM
 * adds nothing for NULLs), pass B counts only the non-NULL vals (the
 * strict COUNT side); groups existing only through NULL vals keep
 * count 0 (a seen key creates its group regardless, execHHashagg
 * find-or-create). */
extern "C" gg_status
gg_engine_hash_groupby_i64_n(const int64_t *keys, const uint8_t *key_nulls,
			     const int64_t *vals, const uint8_t *val_nulls,
			     int64_t n, int64_t *out_keys,
			     int64_t *out_sums, int64_t *out_counts,
			     int64_t cap, int64_t *out_ngroups)
{
	if (!keys || !vals || n < 0 || !out_keys || !out_sums ||
	    !out_counts || !out_ngroups)
		return fail(GG_EINVAL, "bad groupby_n args");
	*out_ngroups = 0;
	std::vector<int64_t> k2((size_t) n), v2((size_t) n);

	for (int64_t i = 0; i < n; i++)
	{
		const bool knull = key_nulls && key_nulls[i];

		if (keys[i] == INT64_MIN)
			return fail(GG_EINVAL,
				    "group key INT64_MIN unsupported");
		/* the NULL group's code: a real key of that value would
		 * merge into the NULL group */
		if (!knull && keys[i] == GG_PLAN_NULL_KEY)
			return fail(GG_EINVAL, "group key INT64_MIN+1 "
				    "(GG_PLAN_NULL_KEY) unsupported");
		k2[i] = knull ? GG_PLAN_NULL_KEY : keys[i];
		v2[i] = (val_nulls && val_nulls[i]) ? 0 : vals[i];
	}
	GG_TRY(gg_engine_hash_groupby_i64(k2.data(), v2.data(), n, out_keys,
					  out_sums, out_counts, cap,
					  out_ngroups));
	if (!val_nulls)
		return GG_OK;

	/* pass B: non-NULL counts via a filtered second group-by */
	std::vector<int64_t> kb, vb;

	kb.reserve((size_t) n);
	for (int64_t i = 0; i < n; i++)
		if (!val_nulls[i])
		{
			kb.push_back(k2[i]);
			vb.push_back(0);
		}
	std::vector<int64_t> bk(kb.size() + 1), bs(kb.size() + 1),
		bc(kb.size() + 1);
	int64_t nb = 0;

	if (!kb.empty())
		GG_TRY(gg_engine_hash_groupby_i64(kb.data(), vb.data(),
						  (int64_t) kb.size(),
						  bk.data(), bs.data(),
						  bc.data(),
						  (int64_t) bk.size(), &nb));
	/* both outputs are sorted by key: merge counts (default 0) */
	{
		int64_t j = 0;

		for (int64_t i = 0; i < *out_ngroups; i++)
		{
			while (j < nb && bk[j] < out_keys[i])
				j++;
			out_counts[i] = (j < nb && bk[j] == out_keys[i])
				? bc[j] : 0;
		}
	}
	return GG_OK;
}

}				/* namespace gg */
