/* Host-only harness: reproduce the plan_rtc codegen for a few plan
 * shapes and dump the generated source (GG_PLAN_RTC_DUMP).
 * hipRTC compiles without a GPU; module load fails afterwards on a
 * CPU-only box, which is fine — the dump is what we want.  Test/dev
 * tooling only; never part of the product path.
 *
 * Build (after the engine library):
 *   hipcc -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
 *     tools/rtc_dump_local.cpp -o tools/rtc_dump_local
 *     -Lgreengage_amd -lgreengage_engine -Wl,-rpath,$PWD/greengage_amd
 *     -L/opt/rocm/lib -lamdhip64
 * Usage: rtc_dump_local [DUMPFILE [SHAPE]]
 *   q1     Q1-shaped grouped plan: generic + baked fast tier (default)
 *   q1w    same, baked 2-word tier
 *   q6     Q6-shaped global-group plan (generic only; never baked)
 *   q1mm   Q1-shaped with MIN/MAX/AVG lowered slots, baked fast tier
 *   q1mmw  same, baked 2-word tier
 *   q6mm   global-group plan with MIN/MAX/AVG lowered slots
 *   gn8    one nullable 8-byte group column; generic + baked 2-word
 *   g4     one 4-byte group column; generic + baked fast tier
 *   join   global-group plan probing one bitmap join and one hash join
 *          with a nullable probe key
 *   pnull  global-group plan with a nullable predicate column
 *   gp     Q1-shaped plan grouped by a packed (int32, nullable int64)
 *          pair: generic + baked fast tier
 *   lrepl  q1mmw's 8 two-word aggregates under GG_PLAN_LREPL=32, which
 *          the LDS budget shrinks back to 16 replicas
 *   q1f    Q1 shape with aggregate filters: sum(price) and
 *          sum(price*(100-disc)) share filter 0 (disc in a range, a column
 *          that is also a factor), COUNT(*) carries filter 1 (qty < k);
 *          generic + baked fast tier
 *   pvf    global-group plan with one dense INNER join whose payload
 *          column feeds two filters over the same SUM factors (a pivot)
 *   left   one group column, a nullable SUM factor and a filter column
 *          from a dense LEFT join's build table, plus a hashed ANTI join
 *          chained through that table; generic + baked 2-word
 *   lefth  global-group plan: hashed LEFT join with a nullable probe key,
 *          ANTI join on a bitmap, SUM(driving x payload), COUNT(payload)
 *   year   plan_outer_bench.py's `year`: dense INNER join, grouped by an
 *          int32 payload column; generic + baked fast tier
 *   yearl  the same with the join made LEFT (`year_left`)
 *   innh   global-group plan: hashed INNER join with a nullable probe key,
 *          and a bitmap ANTI join chained through it whose only condition
 *          is its own nullable probe key
 *   lsemi  dense LEFT join, and a hashed SEMI join chained through it
 *   linner hashed LEFT join, and a dense INNER join chained through it
 *   ll     dense LEFT join, and a dense LEFT join chained through it
 *   lln    the same with the second join hashed on a nullable probe key
 *   wh     Q1 shape with a dense INNER join and WHERE clauses: a scan clause
 *          (disc in a range OR qty <= tax) and a post-join clause over a
 *          nullable payload column; generic + baked fast tier
 *   gc3    Q1 shape grouped by three packed columns (char1, int32, int64)
 *          of the driving table; generic + baked fast tier
 *   gc4    Q1 shape with a dense LEFT join, grouped by four packed columns:
 *          a char1 and a nullable int64 of the driving table, an int32
 *          payload column with a NULL array and a char1 payload column;
 *          generic + baked 2-word
 *   all    every shape above, DUMPFILE used as a prefix: <prefix><shape>.cu
 * Exit status is non-zero when a variant fails to COMPILE (a module
 * load / function lookup failure without a GPU is not a failure). */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../greengage_amd/csrc/engine_internal.h"

using namespace gg;

static char dummy[256];	/* distinct fake pointers per column so the
				 * load-dedup behaves as with real tables */

static void
set_agg(PlanDev &D, int a, int kind, int nf, const int *cols,
	const int *mods)
{
	D.aggs[a].kind = kind;
	D.aggs[a].nf = nf;
	for (int f = 0; f < nf; f++)
	{
		D.aggs[a].col[f] = dummy + cols[f];
		D.aggs[a].width[f] = 8;
		D.aggs[a].mod[f] = (int8_t) mods[f];
	}
}

/* qty/price/disc/tax as four distinct pointers, shared across aggs
 * like the real Q1 plan */
enum { QTY = 24, PRICE = 32, DISC = 40, TAX = 48 };

static void
shape_q1(PlanDev &D, bool mm)
{
	static const int c_q[] = {QTY}, c_p[] = {PRICE}, c_d[] = {DISC};
	static const int c_pd[] = {PRICE, DISC}, c_pdt[] = {PRICE, DISC, TAX};
	static const int m_id[] = {0, 0, 0}, m_pd[] = {0, 1},
		m_pdt[] = {0, 1, 2};

	D.n = 600000000;
	D.npreds = 1;
	D.preds[0].col = dummy + 0;
	D.preds[0].width = 4;
	D.preds[0].lo = -2000000000;
	D.preds[0].hi = 10000;
	D.ngroup = 2;
	D.gcol[0] = dummy + 8;
	D.gcol[1] = dummy + 16;
	D.gwidth[0] = D.gwidth[1] = 1;
	if (!mm)
	{
		/* count, sum(qty), sum(price), sum(disc),
		 * sum(price*(100-disc)), sum(price*(100-disc)*(100+tax)) */
		D.naggs = 6;
		set_agg(D, 0, 0, 0, nullptr, nullptr);
		set_agg(D, 1, 2, 1, c_q, m_id);
		set_agg(D, 2, 2, 1, c_p, m_id);
		set_agg(D, 3, 2, 1, c_d, m_id);
		set_agg(D, 4, 2, 2, c_pd, m_pd);
		set_agg(D, 5, 2, 3, c_pdt, m_pdt);
		return;
	}
	/* count, sum(price*(100-disc)), then the lowered form of
	 * MIN(qty), MAX(price), AVG(disc): value word + non-NULL count,
	 * value word + count, sum + count */
	D.naggs = 8;
	set_agg(D, 0, 0, 0, nullptr, nullptr);
	set_agg(D, 1, 2, 2, c_pd, m_pd);
	set_agg(D, 2, 3, 1, c_q, m_id);
	set_agg(D, 3, 1, 1, c_q, m_id);
	set_agg(D, 4, 4, 1, c_p, m_id);
	set_agg(D, 5, 1, 1, c_p, m_id);
	set_agg(D, 6, 2, 1, c_d, m_id);
	set_agg(D, 7, 1, 1, c_d, m_id);
}

static void
shape_q6(PlanDev &D, bool mm)
{
	static const int c_pd[] = {PRICE, DISC}, c_q[] = {QTY},
		c_p[] = {PRICE};
	static const int m_id[] = {0, 0, 0}, m_sub[] = {1};

	D.n = 600000000;
	D.npreds = 3;
	for (int p = 0; p < 3; p++)
	{
		D.preds[p].col = dummy + 64 + 8 * p;
		D.preds[p].width = p == 0 ? 4 : 8;
		D.preds[p].lo = 0;
		D.preds[p].hi = 10000;
	}
	D.ngroup = 0;
	D.naggs = 2;
	set_agg(D, 0, 2, 2, c_pd, m_id);
	set_agg(D, 1, 0, 0, nullptr, nullptr);
	if (mm)
	{
		D.naggs = 6;
		set_agg(D, 2, 3, 1, c_q, m_sub);
		set_agg(D, 3, 1, 1, c_q, m_id);
		set_agg(D, 4, 4, 1, c_p, m_id);
		set_agg(D, 5, 1, 1, c_p, m_id);
		/* one nullable input so the strict flags are live */
		D.aggs[2].nulls[0] = D.aggs[3].nulls[0] =
			(const uint8_t *) dummy + 128;
	}
}

/* one group column of the given width: count, sum(qty), sum(price*disc) */
static void
shape_g1(PlanDev &D, int width, bool nullable)
{
	static const int c_q[] = {QTY}, c_pd[] = {PRICE, DISC};
	static const int m_id[] = {0, 0, 0};

	shape_q1(D, false);
	D.ngroup = 1;
	D.gcol[1] = nullptr;
	D.gwidth[0] = width;
	D.gwidth[1] = 0;
	if (nullable)
		D.gnulls[0] = (const uint8_t *) dummy + 136;
	D.naggs = 3;
	set_agg(D, 0, 0, 0, nullptr, nullptr);
	set_agg(D, 1, 2, 1, c_q, m_id);
	set_agg(D, 2, 2, 2, c_pd, m_id);
}

/* filter k, conjunct q: lo <= column at dummy + col (of source src) < hi */
static void
set_fpred(PlanDev &D, int k, int q, int col, int width, int src,
	  int64_t lo, int64_t hi)
{
	D.fl.preds[k][q].col = dummy + col;
	D.fl.preds[k][q].width = width;
	D.fl.preds[k][q].lo = lo;
	D.fl.preds[k][q].hi = hi;
	D.fl.psrc[k][q] = (int8_t) src;
	if (D.fl.npreds[k] < q + 1)
		D.fl.npreds[k] = (int8_t) (q + 1);
}

/* slot a carries filter k, as plan.cpp lowers gg_plan_agg.filter */
static void
set_afilt(PlanDev &D, int a, int k)
{
	D.fl.afilt[a] = (int8_t) (1 + k);
	D.fl.used |= 1 << k;
}

/* join j of the given kind probes the `width`-byte column at dummy + 144
 * (join 0) or dummy + 160 (join 1) of source `psrc`; pnulls != 0 makes that
 * key nullable, its flags at dummy + pnulls */
static PlanJoinDev &
set_join(PlanDev &D, int j, int kind, int width, int pnulls = 0, int psrc = 0)
{
	D.njoins = j + 1;
	D.joins[j].pkey = dummy + 144 + 16 * j;
	D.joins[j].width = width;
	if (pnulls)
		D.joins[j].pnulls = (const uint8_t *) dummy + pnulls;
	D.pl.jkind[j] = (int8_t) kind;
	D.pl.jpsrc[j] = (int8_t) psrc;
	if (gg_join_builds_map(kind))
		D.pl.jidx[j] = (const uint32_t *) (dummy + 152);
	return D.joins[j];
}

/* the three build-side structures: a dense key range (INNER / LEFT: index
 * map, SEMI / ANTI: bitmap at dummy + bits) or an open-addressing table */
static void
join_dense(PlanJoinDev &J, int bits = 0)
{
	J.dlen = 1000;
	if (bits)
		J.bits = (const unsigned long long *) (dummy + bits);
}

static void
join_hash(PlanJoinDev &J)
{
	J.hkeys = (const unsigned long long *) (dummy + 176);
	J.hslots = 1024;
}

/* compile errors come back as GG_ENOTSUP with this message prefix */
static bool
compiled(gg_status s)
{
	return s == GG_OK ||
		!std::strstr(gg_engine_last_error(), "compile failed");
}

/* generic kernel, then (nbake > 0) the baked one appended to the dump */
static bool
dump_shape(const char *shape, const char *file)
{
	static const long long q1codes[6] = {16710, 20038, 20050, 33350,
		36934, 33347};
	static const long long g1codes[3] = {3, 1000000007ll,
		GG_PLAN_NULL_KEY};
	bool mm = std::strstr(shape, "mm") != nullptr;
	bool wide = shape[std::strlen(shape) - 1] == 'w';
	const long long *codes = nullptr;
	int nbake = 0;
	PlanDev D{};
	PlanWhereDev W{};
	PlanGroupNDev N{};
	std::shared_ptr<void> out;

	setenv("GG_PLAN_RTC_DUMP", file, 1);
	unsetenv("GG_PLAN_LREPL");
	if (!std::strncmp(shape, "q6", 2))
		shape_q6(D, mm);
	else if (!std::strcmp(shape, "q1f"))
	{
		shape_q1(D, false);
		set_fpred(D, 0, 0, DISC, 8, 0, 5, 8);
		set_fpred(D, 1, 0, QTY, 8, 0, INT64_MIN, 2400);
		set_afilt(D, 2, 0);
		set_afilt(D, 4, 0);
		set_afilt(D, 0, 1);
		codes = q1codes;
		nbake = 6;
	}
	else if (!std::strcmp(shape, "pvf"))
	{
		static const int c_pd[] = {PRICE, DISC};
		static const int m_pd[] = {0, 1};

		shape_q6(D, false);
		D.npreds = 1;
		join_dense(set_join(D, 0, GG_JOIN_INNER, 8));
		D.naggs = 3;
		set_agg(D, 0, 2, 2, c_pd, m_pd);
		set_agg(D, 1, 2, 2, c_pd, m_pd);
		set_agg(D, 2, 2, 2, c_pd, m_pd);
		/* o_orderdate (int32) of the joined orders row, two years */
		set_fpred(D, 0, 0, 200, 4, 1, 8035, 8401);
		set_fpred(D, 1, 0, 200, 4, 1, 8401, 8766);
		set_afilt(D, 0, 0);
		set_afilt(D, 1, 1);
	}
	else if (!std::strncmp(shape, "q1", 2))
	{
		shape_q1(D, mm);
		codes = q1codes;
		nbake = 6;
	}
	else if (!std::strcmp(shape, "gn8") || !std::strcmp(shape, "g4"))
	{
		bool n8 = shape[1] == 'n';

		shape_g1(D, n8 ? 8 : 4, n8);
		wide = n8;
		codes = g1codes;
		nbake = n8 ? 3 : 2;
	}
	else if (!std::strcmp(shape, "join"))
	{
		shape_q6(D, false);
		join_dense(set_join(D, 0, GG_JOIN_SEMI, 8), 152);
		join_hash(set_join(D, 1, GG_JOIN_SEMI, 4, 168));
	}
	else if (!std::strcmp(shape, "left"))
	{
		/* group column, a nullable SUM factor and a filter column from
		 * the build table of a dense LEFT join; a hashed ANTI join
		 * chained through a nullable payload column of it */
		shape_g1(D, 4, false);
		join_dense(set_join(D, 0, GG_JOIN_LEFT, 8));
		join_hash(set_join(D, 1, GG_JOIN_ANTI, 4, 168, 1));
		D.pl.gsrc[0] = 1;
		D.pl.asrc[1][0] = 1;
		D.aggs[1].nulls[0] = (const uint8_t *) dummy + 128;
		D.pl.asrc[2][1] = 1;
		set_fpred(D, 0, 0, 200, 4, 1, 8035, 8401);
		D.fl.preds[0][0].nulls = (const uint8_t *) dummy + 208;
		set_fpred(D, 0, 1, QTY, 8, 1, 0, 2400);
		set_afilt(D, 0, 0);
		wide = true;
		codes = g1codes;
		nbake = 3;
	}
	else if (!std::strcmp(shape, "year") || !std::strcmp(shape, "yearl"))
	{
		/* plan_outer_bench.py's `year` / `year_left`: one dense INNER
		 * (LEFT) join, grouped by an int32 payload column, a SUM over
		 * two driving factors and COUNT(*); generic + baked fast tier */
		static const int c_pd[] = {PRICE, DISC};
		static const int m_pd[] = {0, 1};
		static const long long ycodes[7] = {1992, 1993, 1994, 1995,
			1996, 1997, 1998};

		D.n = 600000000;
		join_dense(set_join(D, 0, shape[4] ? GG_JOIN_LEFT : GG_JOIN_INNER,
				    8));
		D.ngroup = 1;
		D.gcol[0] = dummy + 8;
		D.gwidth[0] = 4;
		D.pl.gsrc[0] = 1;
		D.naggs = 2;
		set_agg(D, 0, 2, 2, c_pd, m_pd);
		set_agg(D, 1, 0, 0, nullptr, nullptr);
		codes = ycodes;
		nbake = 7;
	}
	else if (!std::strcmp(shape, "lefth"))
	{
		/* global-group plan: a hashed LEFT join with a nullable probe
		 * key, an ANTI join on a bitmap, SUM over a driving x payload
		 * product and COUNT(payload) */
		static const int c_pd[] = {PRICE, DISC}, c_q[] = {QTY};
		static const int m_id[] = {0, 0};

		shape_q6(D, false);
		join_hash(set_join(D, 0, GG_JOIN_LEFT, 8, 168));
		join_dense(set_join(D, 1, GG_JOIN_ANTI, 4), 216);
		D.naggs = 3;
		set_agg(D, 0, 2, 2, c_pd, m_id);
		D.pl.asrc[0][1] = 1;
		set_agg(D, 1, 0, 0, nullptr, nullptr);
		set_agg(D, 2, 1, 1, c_q, m_id);
		D.pl.asrc[2][0] = 1;
	}
	else if (!std::strcmp(shape, "innh") || !std::strcmp(shape, "lsemi") ||
		 !std::strcmp(shape, "linner") || !std::strcmp(shape, "ll") ||
		 !std::strcmp(shape, "lln"))
	{
		/* global-group plans whose second join is chained through the
		 * first: SUM(driving x payload of join 0), COUNT(*), and where
		 * join 1 has a payload too, COUNT(payload of join 1) */
		static const int c_pd[] = {PRICE, DISC}, c_q[] = {QTY};
		static const int m_id[] = {0, 0};

		shape_q6(D, false);
		if (!std::strcmp(shape, "innh"))
		{
			join_hash(set_join(D, 0, GG_JOIN_INNER, 8, 168));
			join_dense(set_join(D, 1, GG_JOIN_ANTI, 4, 224, 1), 216);
		}
		else if (!std::strcmp(shape, "lsemi"))
		{
			join_dense(set_join(D, 0, GG_JOIN_LEFT, 8));
			join_hash(set_join(D, 1, GG_JOIN_SEMI, 4, 0, 1));
		}
		else if (!std::strcmp(shape, "linner"))
		{
			join_hash(set_join(D, 0, GG_JOIN_LEFT, 8));
			join_dense(set_join(D, 1, GG_JOIN_INNER, 4, 0, 1));
		}
		else
		{
			join_dense(set_join(D, 0, GG_JOIN_LEFT, 8));
			if (shape[2])
				join_hash(set_join(D, 1, GG_JOIN_LEFT, 4, 224, 1));
			else
				join_dense(set_join(D, 1, GG_JOIN_LEFT, 4, 0, 1));
		}
		D.naggs = 2;
		set_agg(D, 0, 2, 2, c_pd, m_id);
		D.pl.asrc[0][1] = 1;
		set_agg(D, 1, 0, 0, nullptr, nullptr);
		if (D.pl.jidx[1])
		{
			D.naggs = 3;
			set_agg(D, 2, 1, 1, c_q, m_id);
			D.pl.asrc[2][0] = 2;
		}
	}
	else if (!std::strcmp(shape, "pnull"))
	{
		shape_q6(D, false);
		D.preds[1].nulls = (const uint8_t *) dummy + 184;
	}
	else if (!std::strcmp(shape, "gp"))
	{
		static const long long gpcodes[3] = {(1ll << 11) | 1,
			(7ll << 11) | 0, 2000};

		shape_q1(D, false);
		D.gwidth[0] = 4;
		D.gwidth[1] = 8;
		D.gnulls[1] = (const uint8_t *) dummy + 192;
		D.gp.packed = 1;
		D.gp.shift = 11;
		D.gp.gmin[0] = -40;
		D.gp.gmin[1] = 1ll << 50;
		codes = gpcodes;
		nbake = 3;
	}
	else if (!std::strcmp(shape, "wh"))
	{
		shape_q1(D, false);
		join_dense(set_join(D, 0, GG_JOIN_INNER, 8));
		W.atoms[0].col = dummy + DISC;
		W.atoms[0].width = 8;
		W.atoms[0].lo = 5;
		W.atoms[0].hi = 8;
		W.atoms[0].kind = GG_ATOM_RANGE;
		W.atoms[1].col = dummy + QTY;
		W.atoms[1].col2 = dummy + TAX;
		W.atoms[1].width = W.atoms[1].width2 = 8;
		W.atoms[1].kind = GG_ATOM_LE;
		/* o_orderdate (int32) of the joined orders row, nullable */
		W.atoms[2].col = dummy + 200;
		W.atoms[2].nulls = (const uint8_t *) dummy + 208;
		W.atoms[2].width = 4;
		W.atoms[2].src = 1;
		W.atoms[2].lo = 8035;
		W.atoms[2].hi = 8401;
		W.atoms[2].kind = GG_ATOM_NOT_RANGE;
		W.natoms[0] = 2;
		W.natoms[1] = 1;
		W.nclauses = 2;
		W.nscan = 1;
		codes = q1codes;
		nbake = 6;
	}
	else if (!std::strcmp(shape, "gc3"))
	{
		/* fields of 9, 20 and 30 bits */
		static const long long codes3[3] = {
			(67ll << 50) | (5ll << 30) | 12345, (1ll << 50) | 1,
			(80ll << 50) | (1000000ll << 30)};

		shape_q1(D, false);
		D.gwidth[1] = 4;
		N.gcol[0] = dummy + 200;
		N.gwidth[0] = 8;
		N.k.n = 3;
		N.k.shift[0] = 50;
		N.k.shift[1] = 30;
		N.k.gmin[1] = -40;
		N.k.gmin[2] = 1ll << 50;
		codes = codes3;
		nbake = 3;
	}
	else if (!std::strcmp(shape, "gc4"))
	{
		/* fields of 9, 30, 12 and 9 bits; columns 2 and 3 are payload
		 * columns of the LEFT join, NULL on a row without a partner */
		static const long long codes4[3] = {
			(67ll << 51) | (77ll << 21) | (9ll << 9) | 66,
			(67ll << 51) | (77ll << 21), 0};

		shape_q1(D, false);
		join_dense(set_join(D, 0, GG_JOIN_LEFT, 8));
		D.gwidth[1] = 8;
		D.gnulls[1] = (const uint8_t *) dummy + 192;
		N.gcol[0] = dummy + 200;
		N.gwidth[0] = 4;
		N.gnulls[0] = (const uint8_t *) dummy + 208;
		N.gsrc[0] = 1;
		N.gcol[1] = dummy + 224;
		N.gwidth[1] = 1;
		N.gsrc[1] = 1;
		N.k.n = 4;
		N.k.shift[0] = 51;
		N.k.shift[1] = 21;
		N.k.shift[2] = 9;
		N.k.gmin[1] = -(1ll << 28);
		N.k.gmin[2] = 8035;
		wide = true;
		codes = codes4;
		nbake = 3;
	}
	else if (!std::strcmp(shape, "lrepl"))
	{
		setenv("GG_PLAN_LREPL", "32", 1);
		shape_q1(D, true);
		wide = true;
		codes = q1codes;
		nbake = 6;
	}
	else
	{
		fprintf(stderr, "unknown shape %s\n", shape);
		return false;
	}

	bool gn0 = D.gnulls[0] != nullptr, gn1 = D.gnulls[1] != nullptr;
	const PlanWhereDev *Wp = W.nclauses ? &W : nullptr;
	const PlanGroupNDev *Np = N.k.n ? &N : nullptr;
	gg_status s1 = plan_rtc_compile(D, gn0, gn1, &out, nullptr, 0, false, Wp,
					Np);
	bool ok = compiled(s1);

	if (!ok)
		fprintf(stderr, "%s generic: %s\n", shape,
			gg_engine_last_error());
	if (nbake)
	{
		gg_status s2 = plan_rtc_compile(D, gn0, gn1, &out, codes,
						nbake, !wide, Wp, Np);

		if (!compiled(s2))
		{
			fprintf(stderr, "%s baked: %s\n", shape,
				gg_engine_last_error());
			ok = false;
		}
		fprintf(stderr, "%s generic rc=%d baked-%s rc=%d\n", shape,
			s1, wide ? "2word" : "fast", s2);
	}
	else
		fprintf(stderr, "%s generic rc=%d\n", shape, s1);
	return ok;
}

int
main(int argc, char **argv)
{
	static const char *const all[] = {"q1", "q1w", "q6", "q1mm", "q1mmw",
		"q6mm", "gn8", "g4", "join", "pnull", "gp", "lrepl", "q1f", "pvf",
		"left", "lefth", "year", "yearl", "innh", "lsemi", "linner", "ll",
		"lln", "wh", "gc3", "gc4"};
	const char *file = argc > 1 ? argv[1] : "/tmp/rtc_dump.cu";
	const char *shape = argc > 2 ? argv[2] : "q1";
	bool ok = true;

	if (!std::strcmp(shape, "all"))
		for (const char *sh : all)
		{
			std::string f = std::string(file) + sh + ".cu";

			ok = dump_shape(sh, f.c_str()) && ok;
		}
	else
		ok = dump_shape(shape, file);
	fprintf(stderr, "last error: %s\n(a module-load failure is expected "
		"without a GPU)\n", gg_engine_last_error());
	return ok ? 0 : 1;
}
