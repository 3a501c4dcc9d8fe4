/*
 * Runtime kernel specialization for compiled plans (hipRTC).
 *
 * The interpreted generic kernel (plan.hip) pays for its generality in
 * control flow: objdump shows ~6000 instructions with ~790 branches
 * and ~420 s_waitcnt — per-row divergent walks that keep loads from
 * batching (measured 27 G rows/s on a Q1-shaped plan vs 171 G for the
 * hand-specialized kernel).  At gg_engine_compile_plan time we instead
 * GENERATE a gfx950 kernel with the plan's SHAPE baked in — predicate
 * count and column widths, aggregate expression trees, NULL-flag
 * presence, group mode — and JIT it with hipRTC; bounds/constants stay
 * runtime arguments so the same binary serves every execute.  This is
 * the GPU analog of expression compilation the reference executor
 * never had (its ExecQual is interpreted per row, execQual.c:6260).
 *
 * Fallback: any RTC failure leaves the pipeline on the interpreted
 * kernel (stat row path_plan_interp); GG_PLAN_RTC=0 disables JIT.
 */
#include <hip/hiprtc.h>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.h"

namespace gg
{

struct PlanRtc
{
	hipModule_t mod = nullptr;
	hipFunction_t fn = nullptr;

	~PlanRtc()
	{
		if (mod)
			(void) hipModuleUnload(mod);
	}
};

/* The head of every generated program: the text of gg_pg_hash.h and of
 * plan_dev.h (the Makefile writes both into one raw string literal).  The
 * program so sees the very structs, sentinels, hash and accumulator
 * functions the host and plan.hip compile, not a copy of them.  It is
 * concatenated, not passed as a hipRTC header, so a GG_PLAN_RTC_DUMP file
 * is a whole program.  emit_prelude puts the #defines the text expects
 * ahead of it. */
static const char PLAN_DEV_SRC[] =
#include "plan_dev_src.inc"
	;

/* emit a typed, width-baked load; nt = nontemporal streaming load
 * (k_q1_agg measured +11% from NT on its scan columns — the data is
 * touched once per pass, so L2 retention only evicts useful lines) */
static void emit_ld(std::string &s, const char *dst, const char *ptr,
		    int width, const char *idx, bool nt = false)
{
	char buf[256];
	const char *ty = width == 1 ? "const uint8_t *"
		: width == 4 ? "const int32_t *" : "const int64_t *";

	if (nt && width != 1)
		std::snprintf(buf, sizeof(buf),
			      "\t\tint64_t %s = (int64_t) "
			      "__builtin_nontemporal_load(&((%s) %s)[%s]);\n",
			      dst, ty, ptr, idx);
	else
		std::snprintf(buf, sizeof(buf),
			      "\t\tint64_t %s = (int64_t) ((%s) %s)[%s];\n",
			      dst, ty, ptr, idx);
	s += buf;
}

static std::string fmt(const char *f, ...)
	__attribute__((format(printf, 1, 2)));
static std::string fmt(const char *f, ...)
{
	char buf[1024];
	va_list ap;

	va_start(ap, f);
	std::vsnprintf(buf, sizeof(buf), f, ap);
	va_end(ap);
	return buf;
}

/* device helpers only generated kernels use (the group table and the
 * two-word adds are plan_dev.h's); the host emitters below emit CALLS to
 * these, one per accumulator, never their bodies.  All are inlined, so an
 * LDS destination still gets ds_* atomics. */
static const char *DEVICE_FNS = R"GG(
#define LSLOTS 32
#define LEMPTY ((long long) PL_EMPTY)

/* register accumulators: the unsigned max that combines order-encoded
 * MIN/MAX words (0 = identity = "no input") */
__device__ inline void gg_max(unsigned long long &m, unsigned long long v)
{
	if (v > m)
		m = v;
}

/* global-group epilogue: wave-reduce a register accumulator, one global
 * atomic per wave */
__device__ inline void gg_wave_flush_add(unsigned long long *dst,
					 unsigned long long lo,
					 unsigned long long hi)
{
	for (int off = 32; off; off >>= 1)
		pl_add128(lo, hi, __shfl_down(lo, off, 64),
			__shfl_down(hi, off, 64));
	if ((threadIdx.x & 63) == 0 && (lo || hi))
		pl_atomic_add128(dst, lo, hi);
}

__device__ inline void gg_wave_flush_max(unsigned long long *dst,
					 unsigned long long m)
{
	for (int off = 32; off; off >>= 1)
		gg_max(m, __shfl_down(m, off, 64));
	if ((threadIdx.x & 63) == 0 && m)
		atomicMax(dst, m);
}

/* grouped epilogue: fold the LREPL LDS replicas of one accumulator and
 * flush into the global table.  w0 is the accumulator's first word in
 * replica `rr`; the one-word tier is overflow-proven, so its fold needs
 * no carry.  Macros, not functions: as a function the replica loop is
 * unrolled on its own before it is inlined and the flush epilogue then
 * compiles to different code (Q1 baked: 38 instructions and 4 VGPRs
 * less, row loop unchanged); as a macro the program stays
 * instruction-identical to the hand-expanded form it replaces. */
#define GG_FOLD_FLUSH_ADD(dst, w0) \
	do { \
		unsigned long long lo = 0, hi = 0; \
		for (int rr = 0; rr < LREPL; rr++) \
			if (LW == 1) \
				lo += (w0); \
			else \
				pl_add128(lo, hi, (w0), (&(w0))[1]); \
		if (lo || hi) \
			pl_atomic_add128((dst), lo, hi); \
	} while (0)

#define GG_FOLD_FLUSH_MAX(dst, w0) \
	do { \
		unsigned long long m = 0; \
		for (int rr = 0; rr < LREPL; rr++) \
			gg_max(m, (w0)); \
		if (m) \
			atomicMax((dst), m); \
	} while (0)
)GG";

/* everything one generated program is specialized on */
struct Gen
{
	const PlanDev &D;
	bool gnull[2];
	const long long *bake;
	int nbake;
	bool fast;		/* baked one-word tier */
	bool nt;		/* nontemporal scan loads */
	bool payload;		/* the plan holds an INNER or LEFT join: rows
				 * carry the build-row indices r0, r1 */
	const PlanWhereDev *W;	/* scope-0 WHERE clauses, or nullptr */
	const PlanGroupNDev *N;	/* three or four group columns, or nullptr */
};

/* what a launch passes for a plan with WHERE clauses */
struct PlanDevWhere
{
	PlanDev p;
	PlanWhereDev wh;
};

static_assert(offsetof(PlanDevWhere, wh) == sizeof(PlanDev) &&
	      sizeof(PlanDevWhere) == sizeof(PlanDev) + sizeof(PlanWhereDev),
	      "PlanWhereDev follows PlanDev's bytes without padding");

/* ... and for a plan with three or four group columns, with clauses or
 * without (plan_dev.h PlanGroupNDev: the block rides behind `wh`) */
struct PlanDevGroupN
{
	PlanDev p;
	PlanWhereDev wh;
	PlanGroupNDev gn;
};

static_assert(offsetof(PlanDevGroupN, gn) == sizeof(PlanDevWhere) &&
	      sizeof(PlanDevGroupN) == sizeof(PlanDevWhere) +
	      sizeof(PlanGroupNDev),
	      "PlanGroupNDev follows PlanWhereDev's bytes without padding");

/* the plan has clauses evaluated after the joins */
static bool where_post(const Gen &G)
{
	return G.W && G.W->nclauses > G.W->nscan;
}

/* Source `src` is a LEFT join.  Its index r<j> is PL_NOROW on a row the
 * join NULL-extended, and no load may be issued with it: the row carries
 * one `bool h<j>` ("has a partner"), set once where the join is probed,
 * and every use of a column of that source tests it ahead of the address
 * computation: the NULL-flag load and the value load both sit behind it. */
static bool left_src(const PlanDev &D, int src)
{
	return src > 0 && D.pl.jkind[src - 1] == GG_JOIN_LEFT;
}

/* the h<j> parameters of row_pass ("bool &") and agg_vals ("bool "), and
 * with decl = "" the matching call arguments; empty without a LEFT join,
 * so every other plan's program keeps its text */
static std::string left_flags(const PlanDev &D, const char *decl)
{
	std::string s;

	for (int j = 0; j < D.njoins; j++)
		if (D.pl.jkind[j] == GG_JOIN_LEFT)
			s += fmt(", %sh%d", decl, j);
	return s;
}

/* a plan with a packed pair of group columns reads PlanDev.gp; every
 * other plan's program ends PlanDev where it always ended */
static bool packed_args(const PlanDev &D)
{
	return D.ngroup == 2 && D.gp.packed;
}

/* a plan with a referenced aggregate filter reads PlanDev.fl, the last
 * block, and so carries `gp` too */
static bool filter_args(const PlanDev &D)
{
	return D.fl.used != 0;
}

static size_t plan_arg_bytes(const PlanDev &D, const PlanWhereDev *W,
			     const PlanGroupNDev *N)
{
	return N ? sizeof(PlanDevGroupN)
		: W ? sizeof(PlanDevWhere) : filter_args(D) ? sizeof(PlanDev)
		: packed_args(D) ? offsetof(PlanDev, fl) : offsetof(PlanDev, gp);
}

/* the row index a column of source `src` is loaded at: the driving row,
 * or the build row INNER or LEFT join src-1 found for it */
static std::string ix_of(int src)
{
	return src ? fmt("r%d", src - 1) : std::string("i");
}

/* the tail level (plan_dev.h PLAN_DEV_TAIL) of a plan's program */
static int plan_dev_tail(const PlanDev &D, const PlanWhereDev *W,
			 const PlanGroupNDev *N)
{
	return N ? 4 : W ? 3 : filter_args(D) ? 2 : packed_args(D) ? 1 : 0;
}

/* the shared header behind its #defines, layout guards, tunables and the
 * device helpers */
static void emit_prelude(std::string &s, const Gen &G)
{
	const PlanDev &D = G.D;
	const int tail = plan_dev_tail(D, G.W, G.N);
	/* host clang and the amdgcn compiler must agree on every struct the
	 * program's PlanDev holds; `tail` = the lowest level that holds it */
#define GG_LAYOUT(T, tail) {#T, sizeof(T), tail}
	static const struct
	{
		const char *name;
		size_t size;
		int tail;
	} layout[] = {
		GG_LAYOUT(PlanPredDev, 0), GG_LAYOUT(PlanJoinDev, 0),
		GG_LAYOUT(PlanAggDev, 0), GG_LAYOUT(PlanPayloadDev, 0),
		GG_LAYOUT(PlanGroupPackDev, 1), GG_LAYOUT(PlanFilterDev, 2),
		GG_LAYOUT(PlanAtomDev, 3), GG_LAYOUT(PlanWhereDev, 3),
		GG_LAYOUT(PlanKeysN, 4), GG_LAYOUT(PlanGroupNDev, 4)};
#undef GG_LAYOUT

	/* no header can be included under hipRTC: engine_abi.h's bounds go in
	 * as the host compiled them */
#define GG_DEF(M) s += fmt("#define " #M " %d\n", (int) M)
	GG_DEF(GG_PLAN_MAX_PREDS);
	GG_DEF(GG_PLAN_MAX_JOINS);
	GG_DEF(GG_PLAN_MAX_AGGS);
	GG_DEF(GG_PLAN_MAX_FILTERS);
	GG_DEF(GG_PLAN_MAX_FILTER_PREDS);
	GG_DEF(GG_PLAN_MAX_WHERE_ATOMS);
	GG_DEF(GG_PLAN_MAX_CLAUSES);
#undef GG_DEF
	s += fmt("#define PLAN_DEV_TAIL %d\n", tail);
	s += PLAN_DEV_SRC;
	s += "using namespace gg;\n";
	for (const auto &l : layout)
		if (l.tail <= tail)
			s += fmt("static_assert(sizeof(%s) == %zu, \"layout\");\n",
				 l.name, l.size);
	s += fmt("static_assert(sizeof(PlanDev) == %zu, \"layout\");\n",
		 plan_arg_bytes(D, G.W, G.N));

	/* baked variant: more replicas by default — the accumulator
	 * array has only nbake slots, so per-word contention is higher
	 * and LDS is cheap (k_q1_agg makes the same trade) */
	int lrepl = G.nbake > 0 ? 16 : 8;
	const char *lr = getenv("GG_PLAN_LREPL");

	if (lr && atoi(lr) >= 1 && atoi(lr) <= 32)
		lrepl = atoi(lr);
	/* LDS budget: LREPL x slots x 2*naggs u64 must stay within
	 * the per-block share; shrink replicas for wide agg lists */
	{
		int slots = G.nbake > 0 ? G.nbake : 32;

		while (lrepl > 1 &&
		       (size_t) lrepl * slots * 2 * D.naggs * 8 > 64 * 1024)
			lrepl /= 2;
	}
	s += fmt("#define LREPL %d\n", lrepl);
	/* fast (bounds-proven) aggregate values are exact in modular u64
	 * arithmetic — the true per-row value is non-negative < 2^61, so
	 * wrapping intermediates preserve the result and the int128
	 * multiplies (3-4 u64 muls each) collapse to one mul per factor */
	s += G.fast ? "#define VAT unsigned long long\n"
		    : "#define VAT __int128\n";
	/* LW = u64 words per LDS accumulator.  fast (=proven by
	 * plan.cpp's interval bound: every agg value non-negative and
	 * bound*rows_per_block < 2^61) uses ONE word and fire-and-forget
	 * LDS adds — the returned-value carry check otherwise makes
	 * every add a RETURNING atomic, which serializes at the ~88
	 * returning-atomics/us hot-word wall (measured: baked 2-word =
	 * generic 5.5 ms; k_q1_agg's budget-proven 1-word form = 3.6 ms
	 * on the same shape). */
	s += G.fast ? "#define LW 1\n" : "#define LW 2\n";
	{
		/* a filtered aggregate's flag starts from its filter */
		bool nn = !filter_args(D);

		for (int a = 0; a < D.naggs; a++)
			for (int f = 0; f < D.aggs[a].nf; f++)
				if (D.aggs[a].nulls[f] ||
				    left_src(D, D.pl.asrc[a][f]))
					nn = false;
		/* strict-transition flags vanish at compile time when
		 * no aggregate input is nullable (a column of a LEFT
		 * join's build table always is) and no aggregate is
		 * filtered (the common case) */
		s += nn ? "#define AOK(a) true\n"
			: "#define AOK(a) (aok[a])\n";
	}
	s += DEVICE_FNS;
}

/* ---- one join of the row filter ----
 * The open-addressing probe of P.joins[<j>] (J) for key k<j> (k): keys are
 * stored as key ^ msb, 0 = empty.  `hit` and `miss` are the statements on a
 * matching and on an empty slot, `after` the text behind the loop.  With
 * empty_first a probe key of INT64_MIN (encoded 0 = the empty sentinel)
 * finds nothing and never reads an unwritten index */
static void emit_hash_probe(std::string &s, const std::string &k,
			    const std::string &J, bool empty_first,
			    const std::string &hit, const std::string &miss,
			    const std::string &after = "")
{
	const std::string e = "\t\t\t\tif (cur == 0) " + miss + "\n";
	const std::string m = "\t\t\t\tif (cur == t) " + hit + "\n";

	s += "\t\t{\n\t\t\tunsigned long long t = (unsigned long long) " + k +
		" ^ PL_MSB;\n\t\t\tuint64_t pos = (uint64_t) "
		"gg_hashint8(" + k + ") & (" + J + ".hslots - 1);\n"
		"\t\t\tfor (;;) {\n\t\t\t\tunsigned long long cur = " + J +
		".hkeys[pos];\n" + (empty_first ? e + m : m + e) +
		"\t\t\t\tpos = (pos + 1) & (" + J + ".hslots - 1);\n\t\t\t}\n" +
		after + "\t\t}\n";
}

static void emit_join(std::string &s, const PlanDev &D, int j)
{
	const int kind = D.pl.jkind[j], ps = D.pl.jpsrc[j];
	const bool map = gg_join_builds_map(kind);
	const bool keep = gg_join_keeps_unmatched(kind);
	const std::string pi = ix_of(ps), k = fmt("k%d", j), r = fmt("r%d", j),
		J = fmt("P.joins[%d]", j), take = r + fmt(" = P.pl.jidx[%d]", j),
		in = k + " >= 0 && " + k + " < " + J + ".dlen",
		out = k + " < 0 || " + k + " >= " + J + ".dlen", no = "return false;";
	/* The probe key is NULL where its source, an earlier LEFT join,
	 * NULL-extended the row (hs clear), or by its own flag nf; the source
	 * is tested first, which keeps the flag load behind it.  SEMI and INNER
	 * drop such a row (NULL never matches); LEFT and ANTI skip the probe:
	 * LEFT NULL-extends and ANTI keeps the row */
	const std::string hs = left_src(D, ps) ? fmt("h%d", ps - 1) : "",
		nf = D.joins[j].pnulls ? J + ".pnulls[" + pi + "]" : "";

	if (kind == GG_JOIN_LEFT)
		s += "\t\t" + r + " = PL_NOROW;\n";
	if (!keep)
		s += (hs.empty() ? "" : "\t\tif (!" + hs + ") " + no + "\n") +
			(nf.empty() ? "" : "\t\tif (" + nf + ") " + no + "\n");
	else if (hs.empty() && nf.empty())
		s += "\t\t{\n";
	else
		s += "\t\tif (" + hs + (hs.empty() || nf.empty() ? "" : " && ") +
			(nf.empty() ? "" : "!" + nf) + ")\n\t\t{\n";
	/* a gathered probe key (chained join) is never streamed */
	emit_ld(s, k.c_str(), (J + ".pkey").c_str(), D.joins[j].width,
		pi.c_str());
	if (map && D.joins[j].dlen)
		/* dense index map: the range check comes before the map is
		 * touched; PL_NOROW = no build row, LEFT's "no partner" */
		s += keep ? "\t\tif (" + in + ")\n\t\t\t" + take + "[" + k + "];\n"
			: "\t\tif (" + out + ")\n\t\t\t" + no + "\n\t\t" + take + "[" +
			  k + "];\n\t\tif (" + r + " == PL_NOROW) " + no + "\n";
	else if (!map && D.joins[j].bits)
		/* SEMI drops a non-member; ANTI is the same test, inverted */
		s += "\t\tif (" + (keep ? in + " &&" : out + " ||") + "\n\t\t    " +
			(keep ? "" : "!") + "((" + J + ".bits[" + k + " >> 6] >> (" +
			k + " & 63)) & 1))\n\t\t\t" + no + "\n";
	else if (kind == GG_JOIN_SEMI)
		/* match before empty, as ever: an INT64_MIN probe key "matches"
		 * the first empty slot (LEFT OUTER and ANTI joins) */
		emit_hash_probe(s, k, J, false, "break;", no);
	else if (kind == GG_JOIN_INNER)
		emit_hash_probe(s, k, J, true, "break;", no,
				"\t\t\t" + take + "[pos];\n");
	else if (kind == GG_JOIN_LEFT)
		emit_hash_probe(s, k, J, true, "{ " + take + "[pos]; break; }",
				"break;");
	else
		emit_hash_probe(s, k, J, true, no, "break;");
	if (kind == GG_JOIN_LEFT)
		/* close the probe, then the row's one "has a partner" flag */
		s += "\t\t}\n\t\th" + std::to_string(j) + " = " + r +
			" != PL_NOROW;\n";
	else if (keep)
		s += "\t\t}\n";
}

/* ---- general WHERE clauses (engine_abi.h gg_plan_where) ----
 * "Column x of source src is SQL NULL" as program text, "" = never: by its
 * own flag array `nptr`, or, for a LEFT source, on a NULL-extended row.
 * The partner flag h<j> comes first, and `||` / `&&` keep the flag load
 * behind it. */
static std::string atom_isnull(const PlanDev &D, int src, bool has_nulls,
			       const std::string &nptr)
{
	const std::string f = has_nulls ? nptr + "[" + ix_of(src) + "]" : "";

	if (left_src(D, src))
		return f.empty() ? fmt("!h%d", src - 1)
			: fmt("(!h%d || ", src - 1) + f + ")";
	return f;
}

static std::string atom_notnull(const PlanDev &D, int src, bool has_nulls,
				const std::string &nptr)
{
	const std::string f = has_nulls ? nptr + "[" + ix_of(src) + "]" : "";

	if (left_src(D, src))
		return f.empty() ? fmt("h%d", src - 1)
			: fmt("(h%d && !", src - 1) + f + ")";
	return f.empty() ? f : "!" + f;
}

/* Atom q of P.wh as a branch-free boolean over its loaded values va / vb.
 * Kind, widths and NULL presence are baked, the bounds stay arguments.  A
 * comparison over a NULL is not true; IS_NULL is true exactly then. */
static std::string atom_expr(const PlanDev &D, const PlanAtomDev &A, int q,
			     const std::string &va, const std::string &vb)
{
	const std::string P = fmt("P.wh.atoms[%d]", q);
	const char *a = va.c_str(), *b = vb.c_str(), *p = P.c_str();
	std::string e;

	if (A.kind >= GG_ATOM_IS_NULL)
	{
		e = atom_isnull(D, A.src, A.nulls != nullptr, P + ".nulls");
		if (A.kind == GG_ATOM_IS_NULL)
			return e.empty() ? "false" : "(bool) " + e;
		return e.empty() ? "true" : "!" + e;
	}
	switch (A.kind)
	{
		case GG_ATOM_RANGE:
			e = fmt("(%s >= %s.lo) & (%s < %s.hi)", a, p, a, p);
			break;
		case GG_ATOM_NOT_RANGE:
			e = fmt("((%s < %s.lo) | (%s >= %s.hi))", a, p, a, p);
			break;
		default:
			e = fmt("(%s %s %s)", a, A.kind == GG_ATOM_LT ? "<"
				: A.kind == GG_ATOM_LE ? "<="
				: A.kind == GG_ATOM_EQ ? "==" : "!=", b);
	}
	const std::string na = atom_notnull(D, A.src, A.nulls != nullptr,
					    P + ".nulls");
	const std::string nb = A.col2
		? atom_notnull(D, A.src2, A.nulls2 != nullptr, P + ".nulls2") : "";

	return "(" + e + (na.empty() ? "" : " & " + na) +
		(nb.empty() ? "" : " & " + nb) + ")";
}

/* clauses [c0, c1) of P.wh: per clause the loads of its atoms' columns
 * (value_of names the variable holding a column, emitting the load on first
 * use), then one test: a clause none of whose atoms is true drops the row */
template <class ValueOf>
static void emit_where_clauses(std::string &s, const Gen &G, int c0, int c1,
			       ValueOf value_of)
{
	const PlanWhereDev &W = *G.W;
	int q = 0;

	for (int c = 0; c < c1; c++)
	{
		std::string e;

		for (const int end = q + W.natoms[c]; q < end; q++)
		{
			const PlanAtomDev &A = W.atoms[q];
			std::string va, vb;

			if (c < c0)
				continue;
			if (A.kind < GG_ATOM_IS_NULL)
				va = value_of(A.col, A.width, A.src,
					      fmt("P.wh.atoms[%d].col", q));
			if (A.col2)
				vb = value_of(A.col2, A.width2, A.src2,
					      fmt("P.wh.atoms[%d].col2", q));
			e += (e.empty() ? "" : "\n\t\t      | ") +
				atom_expr(G.D, A, q, va, vb);
		}
		if (c >= c0)
			s += "\t\tif (!(" + e + ")) return false;\n";
	}
}

/* ---- per-row evaluation as a macro-free inline sequence ---- */
static void emit_row_pass(std::string &s, const Gen &G)
{
	const PlanDev &D = G.D;

	s += G.payload
		? fmt("\tauto row_pass = [&](int64_t i, uint32_t &r0, uint32_t &r1%s)"
		      " -> bool\n\t{\n", left_flags(D, "bool &").c_str())
		: "\tauto row_pass = [&](int64_t i) -> bool\n\t{\n";
	for (int p = 0; p < D.npreds; p++)
	{
		emit_ld(s, fmt("v%d", p).c_str(),
			fmt("P.preds[%d].col", p).c_str(), D.preds[p].width,
			"i", G.nt);
		if (D.preds[p].nulls)
			s += fmt("\t\tif (P.preds[%d].nulls[i]) return false;\n",
				 p);
		s += fmt("\t\tif (v%d < P.preds[%d].lo || v%d >= P.preds[%d].hi) return false;\n",
			 p, p, p, p);
	}
	if (G.W && G.W->nscan)
	{
		/* scan clauses, ahead of the joins.  Every atom reads the
		 * driving row; a column a pred or an earlier atom loaded is
		 * not loaded again (an IN-list is one load and n compares) */
		struct Ld
		{
			const void *col;
			int width;
			std::string var;
		};
		std::vector<Ld> have;

		for (int p = 0; p < D.npreds; p++)
			have.push_back({D.preds[p].col, D.preds[p].width,
					fmt("v%d", p)});
		emit_where_clauses(s, G, 0, G.W->nscan,
				   [&](const void *c, int w, int,
				       const std::string &ptr) -> std::string
		{
			for (auto &h : have)
				if (h.col == c && h.width == w)
					return h.var;
			have.push_back({c, w, fmt("w%d", (int) have.size())});
			emit_ld(s, have.back().var.c_str(), ptr.c_str(), w, "i",
				G.nt);
			return have.back().var;
		});
	}
	for (int j = 0; j < D.njoins; j++)
		emit_join(s, D, j);
	s += "\t\treturn true;\n\t};\n";
}

/* agg input values.  Factor-column loads are DEDUPLICATED at
 * generation time: the same device pointer can appear in many
 * aggregates (Q1 reads price in three sums) and clang cannot
 * prove P.aggs[i].col[f] aliases across aggs, so without this
 * the kernel issued 13 per-row VMEM loads where the
 * hand-written k_q1_agg issues 7 (measured via offline ISA
 * dump, tools/rtc_dump_local.cpp).  A load is one (pointer, width,
 * source): a table joined twice as INNER is two sources, and its
 * columns are then read at two different build rows.
 *
 * Aggregate filters (PlanFilterDev): their predicate columns go through
 * the same load table, so a column that is both a factor and a filter
 * input is loaded once; each referenced filter k becomes one branch-free
 * `bool flt<k>` per row, and a filtered aggregate's aok[a] starts from
 * it instead of `true`.  emit_transitions gates every destination on
 * AOK(a), so nothing downstream knows about filters. */
static void emit_agg_vals(std::string &s, const Gen &G)
{
	const PlanDev &D = G.D;
	struct Ld
	{
		const void *col;
		int width, src;
	};
	std::vector<Ld> uniq;
	auto var_ld = [&](const void *c, int w, int src,
			  const std::string &ptr) -> int
	{
		for (size_t u = 0; u < uniq.size(); u++)
			if (uniq[u].col == c && uniq[u].width == w &&
			    uniq[u].src == src)
				return (int) u;
		uniq.push_back({c, w, src});
		if (left_src(D, src))
		{
			/* a LEFT-source column: loaded behind the row's
			 * partner flag, 0 on a NULL-extended row (whose every
			 * user is switched off by the same flag) */
			s += fmt("\t\tint64_t xu%d = 0;\n\t\tif (h%d)\n"
				 "\t\t\txu%d = (int64_t) ((%s) %s)[%s];\n",
				 (int) uniq.size() - 1, src - 1,
				 (int) uniq.size() - 1,
				 w == 1 ? "const uint8_t *"
				 : w == 4 ? "const int32_t *" : "const int64_t *",
				 ptr.c_str(), ix_of(src).c_str());
			return (int) uniq.size() - 1;
		}
		emit_ld(s, fmt("xu%d", (int) uniq.size() - 1).c_str(),
			ptr.c_str(), w, ix_of(src).c_str(),
			/* gathered payload loads are never nontemporal */
			G.nt && !src);
		return (int) uniq.size() - 1;
	};
	auto var_of = [&](int a, int f) -> int
	{
		return var_ld(D.aggs[a].col[f], D.aggs[a].width[f],
			      D.pl.asrc[a][f],
			      fmt("P.aggs[%d].col[%d]", a, f));
	};
	/* the factor as it enters a product: the loaded var or its
	 * (100±) term */
	auto term_of = [&](int a, int f) -> std::string
	{
		int u = var_of(a, f);

		return D.aggs[a].mod[f]
			? fmt("xm%d_%d", u, (int) D.aggs[a].mod[f])
			: fmt("xu%d", u);
	};

	/* with post-join WHERE clauses the lambda answers "the row survives" */
	const char *ret = where_post(G) ? " -> bool" : "";

	s += G.payload
		? fmt("\tauto agg_vals = [&](int64_t i, uint32_t r0, uint32_t r1%s, "
		      "VAT *av, bool *aok)%s\n\t{\n",
		      left_flags(D, "bool ").c_str(), ret)
		: fmt("\tauto agg_vals = [&](int64_t i, VAT *av, bool *aok)%s\n\t{\n",
		      ret);
	/* pass 0: the post-join WHERE clauses, through the load table below,
	 * so a column that is an atom, a factor and a filter input is loaded
	 * once; a row they drop leaves before any other load */
	if (where_post(G))
		emit_where_clauses(s, G, G.W->nscan, G.W->nclauses,
				   [&](const void *c, int w, int src,
				       const std::string &ptr) -> std::string
		{
			return fmt("xu%d", var_ld(c, w, src, ptr));
		});
	/* pass 1: one load per distinct (pointer, width) */
	for (int a = 0; a < D.naggs; a++)
		if (D.aggs[a].kind >= 2)
			for (int f = 0; f < D.aggs[a].nf; f++)
				(void) var_of(a, f);
	/* pass 1b: each distinct (var, 100±) term once — (100-disc)
	 * feeds two of Q1's sums */
	{
		std::vector<std::pair<int, int>> mods_done;

		for (int a = 0; a < D.naggs; a++)
			if (D.aggs[a].kind >= 2)
				for (int f = 0; f < D.aggs[a].nf; f++)
				{
					int m = D.aggs[a].mod[f];

					if (!m)
						continue;
					int u = var_of(a, f);
					bool seen = false;

					for (auto &q : mods_done)
						if (q.first == u &&
						    q.second == m)
							seen = true;
					if (seen)
						continue;
					mods_done.push_back({u, m});
					s += fmt("\t\tint64_t xm%d_%d = 100 %c xu%d;\n",
						 u, m, m == 1 ? '-' : '+', u);
				}
	}
	/* pass 1c: every referenced filter once, branch-free like the
	 * strided predicate streams: range test on the loaded value, AND the
	 * NULL flag where the column has one (the value under a set flag is
	 * loaded and ignored) */
	for (int k = 0; k < GG_PLAN_MAX_FILTERS; k++)
	{
		if (!((D.fl.used >> k) & 1))
			continue;
		std::string e;

		for (int q = 0; q < D.fl.npreds[k]; q++)
		{
			const PlanPredDev &F = D.fl.preds[k][q];
			int src = D.fl.psrc[k][q];
			int u = var_ld(F.col, F.width, src,
				       fmt("P.fl.preds[%d][%d].col", k, q));

			e += fmt("%s(xu%d >= P.fl.preds[%d][%d].lo) & "
				 "(xu%d < P.fl.preds[%d][%d].hi)",
				 q ? "\n\t\t\t& " : "", u, k, q, u, k, q);
			if (left_src(D, src))
				/* NULL-extended: the conjunct is not true; `&&`
				 * keeps the flag load behind the partner flag */
				e += F.nulls
					? fmt(" & (h%d && !P.fl.preds[%d][%d].nulls[%s])",
					      src - 1, k, q, ix_of(src).c_str())
					: fmt(" & h%d", src - 1);
			else if (F.nulls)
				e += fmt(" & !P.fl.preds[%d][%d].nulls[%s]", k, q,
					 ix_of(src).c_str());
		}
		s += fmt("\t\tbool flt%d = %s;\n", k, e.c_str());
	}
	/* the flag an aggregate's strict rule starts from */
	auto aok0 = [&](int a) -> std::string
	{
		return D.fl.afilt[a] ? fmt("flt%d", D.fl.afilt[a] - 1)
			: std::string("true");
	};

	/* pass 2: per-agg strict flags + products over the shared vars */
	for (int a = 0; a < D.naggs; a++)
	{
		if (D.aggs[a].kind == 0)
		{
			s += fmt("\t\tav[%d] = 1; aok[%d] = %s;\n", a, a,
				 aok0(a).c_str());
			continue;
		}
		s += fmt("\t\taok[%d] = %s;\n", a, aok0(a).c_str());
		for (int f = 0; f < D.aggs[a].nf; f++)
			if (left_src(D, D.pl.asrc[a][f]))
				/* strict: a NULL-extended factor is skipped */
				s += D.aggs[a].nulls[f]
					? fmt("\t\tif (!h%d || P.aggs[%d].nulls[%d][%s]) aok[%d] = false;\n",
					      D.pl.asrc[a][f] - 1, a, f,
					      ix_of(D.pl.asrc[a][f]).c_str(), a)
					: fmt("\t\tif (!h%d) aok[%d] = false;\n",
					      D.pl.asrc[a][f] - 1, a);
			else if (D.aggs[a].nulls[f])
				s += fmt("\t\tif (P.aggs[%d].nulls[%d][%s]) aok[%d] = false;\n",
					 a, f, ix_of(D.pl.asrc[a][f]).c_str(),
					 a);
		if (D.aggs[a].kind == 1)
			s += fmt("\t\tav[%d] = 1;\n", a);
		else if (D.aggs[a].kind >= 3)
			/* MIN/MAX word: order-encode AFTER the modifier so
			 * unsigned max combines both (MAX: x ^ msb, MIN:
			 * its complement; 0 = identity = "no input") */
			s += fmt("\t\tav[%d] = (VAT) %s((unsigned long long) %s"
				 " ^ PL_MSB);\n",
				 a, D.aggs[a].kind == 3 ? "~" : "",
				 term_of(a, 0).c_str());
		else
		{
			s += "\t\t{ VAT v = 1;\n";
			for (int f = 0; f < D.aggs[a].nf; f++)
				s += fmt("\t\tv *= (VAT) %s;\n",
					 term_of(a, f).c_str());
			s += fmt("\t\tav[%d] = v; }\n", a);
		}
	}
	s += where_post(G) ? "\t\treturn true;\n\t};\n" : "\t};\n";
}

/* the scan loop's head, shared by every variant: filter, group code
 * (grouped plans), aggregate inputs */
static void emit_loop_head(std::string &s, const Gen &G)
{
	const PlanDev &D = G.D;
	static const char *const ld[] = {
		"(long long) ((const uint8_t *) P.gcol[%d])[%s]",
		"(long long) ((const int32_t *) P.gcol[%d])[%s]",
		"((const int64_t *) P.gcol[%d])[%s]"};
	std::string gi[2] = {ix_of(D.pl.gsrc[0]), ix_of(D.pl.gsrc[1])};
	static const char *const ldn[] = {
		"(long long) ((const uint8_t *) %s)[%s]",
		"(long long) ((const int32_t *) %s)[%s]",
		"((const int64_t *) %s)[%s]"};

	s += R"GG(
	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < P.n; i += stride)
	{
)GG";
	std::string hdecl;

	for (int j = 0; j < D.njoins; j++)
		if (D.pl.jkind[j] == GG_JOIN_LEFT)
			hdecl += fmt("\t\tbool h%d = false;\n", j);
	s += G.payload
		? fmt("\t\tuint32_t r0 = 0, r1 = 0;\n%s\n"
		      "\t\tif (!row_pass(i, r0, r1%s))\n\t\t\tcontinue;\n",
		      hdecl.c_str(), left_flags(D, "").c_str())
		: "\t\tif (!row_pass(i))\n\t\t\tcontinue;\n";
	/* a group column is NULL by its own flag or, for a LEFT source, on a
	 * NULL-extended row; `||` keeps the flag load and the ternary the
	 * value load behind the partner flag */
	bool gn[2] = {false, false};
	std::string gc[2];

	for (int g = 0; g < D.ngroup; g++)
	{
		const bool ls = left_src(D, D.pl.gsrc[g]);

		gn[g] = G.gnull[g] || ls;
		gc[g] = !ls ? fmt("P.gnulls[%d][%s]", g, gi[g].c_str())
			: G.gnull[g] ? fmt("(!h%d || P.gnulls[%d][%s])",
					   D.pl.gsrc[g] - 1, g, gi[g].c_str())
			: fmt("!h%d", D.pl.gsrc[g] - 1);
	}
	if (G.N)
	{
		/* three or four packed fields (plan_dev.h PlanKeysN): e_g as in
		 * the packed pair below; the load widths, NULL presence and the
		 * shifts are baked, the minima stay arguments */
		std::string code;

		for (int g = 0; g < G.N->k.n; g++)
		{
			const PlanGroupCol C = plan_group_col(D, *G.N, g);
			const int src = C.src, w = C.width;
			/* columns 0 and 1: NULL presence as the caller baked it */
			const bool hasn = g < 2 ? G.gnull[g] : C.nulls != nullptr;
			const bool ls = left_src(D, src);
			const std::string ix = ix_of(src),
				col = g < 2 ? fmt("P.gcol[%d]", g)
				: fmt("P.gn.gcol[%d]", g - 2),
				nf = (g < 2 ? fmt("P.gnulls[%d]", g)
				      : fmt("P.gn.gnulls[%d]", g - 2)) + "[" + ix + "]",
				isnull = !ls ? nf
				: hasn ? fmt("(!h%d || ", src - 1) + nf + ")"
				: fmt("!h%d", src - 1);
			std::string e = fmt(ldn[w == 1 ? 0 : w == 4 ? 1 : 2],
					    col.c_str(), ix.c_str());

			e = fmt("(unsigned long long) (%s) - (unsigned long long) "
				"P.gn.k.gmin[%d] + 1ull", e.c_str(), g);
			if (hasn || ls)
				e = isnull + " ? 0ull : " + e;
			s += fmt("\t\tunsigned long long e%d = %s;\n", g, e.c_str());
			code += fmt("%s(e%d << %d)", g ? " | " : "", g,
				    G.N->k.shift[g]);
		}
		s += "\t\tlong long code = (long long) (" + code + ");\n";
	}
	else if (packed_args(D))
	{
		/* packed pair (engine_abi.h gg_plan_desc.group_cols): e = 0
		 * for NULL, else v - min + 1 in unsigned arithmetic; the
		 * load widths, NULL presence and the shift are baked, the
		 * minima stay arguments */
		for (int g = 0; g < 2; g++)
		{
			std::string e = fmt(ld[D.gwidth[g] == 1 ? 0
					       : D.gwidth[g] == 4 ? 1 : 2], g,
					    gi[g].c_str());

			e = fmt("(unsigned long long) (%s) - (unsigned long long) "
				"P.gp.gmin[%d] + 1ull", e.c_str(), g);
			if (gn[g])
				e = fmt("%s ? 0ull : %s", gc[g].c_str(), e.c_str());
			s += fmt("\t\tunsigned long long e%d = %s;\n", g,
				 e.c_str());
		}
		s += fmt("\t\tlong long code = (long long) ((e0 << %d) | e1);\n",
			 D.gp.shift);
	}
	else if (D.ngroup == 2)
	{
		/* two char1 columns; NULL encodes as 256 */
		for (int g = 0; g < 2; g++)
		{
			std::string e = fmt(ld[0], g, gi[g].c_str());

			if (gn[g])
				e = fmt("(%s ? 256 : %s)", gc[g].c_str(), e.c_str());
			s += fmt("\t\tlong long e%d = %s;\n", g, e.c_str());
		}
		s += "\t\tlong long code = e0 * 512 + e1;\n";
	}
	else if (D.ngroup == 1)
	{
		std::string e = fmt(ld[D.gwidth[0] == 1 ? 0
				       : D.gwidth[0] == 4 ? 1 : 2], 0,
				    gi[0].c_str());

		if (gn[0])
			e = gc[0] + " ? (long long) "
				"0x8000000000000001ull : (" + e + ")";
		s += "\t\tlong long code = " + e + ";\n";
	}
	s += R"GG(
		VAT av[NA];
		bool aok[NA];

)GG";
	const std::string call = G.payload
		? fmt("agg_vals(i, r0, r1%s, av, aok)", left_flags(D, "").c_str())
		: "agg_vals(i, av, aok)";

	/* a post-join WHERE clause drops the row before it touches a group */
	s += where_post(G) ? "\t\tif (!" + call + ")\n\t\t\tcontinue;\n"
		: "\t\t" + call + ";\n";
}

/* where a row's transition lands */
enum Dest
{
	DEST_REG,		/* registers alo[a] / ahi[a] */
	DEST_LDS,		/* generic block cache lvals[lrep][ls][..] */
	DEST_BAKED,		/* baked table mine[..], LW words */
	DEST_GLOBAL		/* P.tvals[(slot * NA + a) * 2] */
};

/* av[a] into accumulator a at `dest`, once per accumulator from its
 * kind: the kinds are known here, so the row loop carries no kind
 * branch.  MIN/MAX words take the (non-returning) unsigned max, the
 * one-word tier a fire-and-forget add, everything else the two-word
 * add with carry. */
static void emit_transitions(std::string &s, const Gen &G, const char *ind,
			     Dest dest)
{
	static const char *const word0[] = {
		"alo[%d]", "lvals[lrep][ls][2 * %d]",
		"mine[(g * NA + %d) * LW]", "P.tvals[(slot * NA + %d) * 2]"};

	for (int a = 0; a < G.D.naggs; a++)
	{
		std::string w = fmt(word0[dest], a);
		std::string v = fmt("(unsigned long long) av[%d]", a);
		std::string call;

		if (G.D.aggs[a].kind >= 3)
			call = dest == DEST_REG
				? fmt("gg_max(%s, %s)", w.c_str(), v.c_str())
				: fmt("atomicMax(&%s, %s)", w.c_str(), v.c_str());
		else if (dest == DEST_BAKED && G.fast)
			call = fmt("atomicAdd(&%s, %s)", w.c_str(), v.c_str());
		else if (dest == DEST_REG)
			call = fmt("pl_add128(%s, ahi[%d], %s, "
				   "(unsigned long long) (av[%d] >> 64))",
				   w.c_str(), a, v.c_str(), a);
		else
			call = fmt("pl_atomic_add128(&%s, %s, "
				   "(unsigned long long) (av[%d] >> 64))",
				   w.c_str(), v.c_str(), a);
		s += fmt("%sif (AOK(%d))\n%s\t%s;\n", ind, a, ind,
			 call.c_str());
	}
}

/* fold the LREPL replicas of every accumulator of LDS group q (word0:
 * accumulator a's first word in replica rr) into global slot `slot` */
static void emit_flushes(std::string &s, const Gen &G, const char *word0)
{
	for (int a = 0; a < G.D.naggs; a++)
		s += fmt("\t\tGG_FOLD_FLUSH_%s(&P.tvals[(slot * NA + %d) * 2], %s);\n",
			 G.D.aggs[a].kind >= 3 ? "MAX" : "ADD", a,
			 fmt(word0, a).c_str());
}

/* no group columns: register accumulators, one wave-reduced global
 * atomic per wave and accumulator */
static void emit_body_global(std::string &s, const Gen &G)
{
	s += "\tunsigned long long alo[NA] = {};\n"
	     "\tunsigned long long ahi[NA] = {};\n";
	emit_loop_head(s, G);
	emit_transitions(s, G, "\t\t", DEST_REG);
	s += "\t}\n";
	for (int a = 0; a < G.D.naggs; a++)
		if (G.D.aggs[a].kind >= 3)
			s += fmt("\tgg_wave_flush_max(&P.tvals[2 * %d], alo[%d]);\n",
				 a, a);
		else
			s += fmt("\tgg_wave_flush_add(&P.tvals[2 * %d], alo[%d], ahi[%d]);\n",
				 a, a, a);
	s += R"GG(	if (blockIdx.x == 0 && threadIdx.x == 0)
		P.tkeys[0] = 0;
)GG";
}

/* grouped, group set unknown: per-block LDS find-or-create cache in
 * front of the global table */
static void emit_body_grouped(std::string &s, const Gen &G)
{
	s += R"GG(
	__shared__ long long lkeys[LSLOTS];
	__shared__ unsigned long long lvals[LREPL][LSLOTS][2 * NA];

	for (int q = threadIdx.x; q < LSLOTS; q += blockDim.x)
		lkeys[q] = LEMPTY;
	for (int q = threadIdx.x; q < LREPL * LSLOTS * 2 * NA;
	     q += blockDim.x)
		((unsigned long long *) lvals)[q] = 0;
	__syncthreads();
	const int lrep = (int) (threadIdx.x & (LREPL - 1));
)GG";
	emit_loop_head(s, G);
	s += R"GG(		int ls = -1;
		uint32_t pos = (uint32_t) gg_hashint8(code) & (LSLOTS - 1);

		for (int probe = 0; probe < 8; probe++)
		{
			long long cur = lkeys[pos];

			if (cur == code) { ls = (int) pos; break; }
			if (cur == LEMPTY)
			{
				long long prev = atomicCAS(
					(unsigned long long *) &lkeys[pos],
					(unsigned long long) LEMPTY,
					(unsigned long long) code);

				if (prev == LEMPTY || prev == code)
				{ ls = (int) pos; break; }
				continue;
			}
			pos = (pos + 1) & (LSLOTS - 1);
		}
		if (ls >= 0)
		{
)GG";
	emit_transitions(s, G, "\t\t\t", DEST_LDS);
	s += R"GG(		}
		else
		{
			int64_t slot = pl_slot(P, code);

			if (slot < 0) { atomicOr(P.err, PL_ERR_FULL); continue; }
)GG";
	emit_transitions(s, G, "\t\t\t", DEST_GLOBAL);
	s += R"GG(		}
	}
	__syncthreads();
	for (int q = threadIdx.x; q < LSLOTS; q += blockDim.x)
	{
		if (lkeys[q] == LEMPTY)
			continue;
		int64_t slot = pl_slot(P, lkeys[q]);

		if (slot < 0) { atomicOr(P.err, PL_ERR_FULL); continue; }
)GG";
	emit_flushes(s, G, "lvals[rr][q][2 * %d]");
	s += "\t}\n";
}

/* ---- baked-codes variant ----------------------
 * The group set was observed on a prior execute
 * of this plan (tables are immutable, so it is
 * exact for repeats).  Codes become a constexpr
 * compare chain -> direct LDS index: no key
 * probe, no CAS on the hot path.  A row whose
 * code is not baked (impossible for repeats,
 * kept for correctness) is counted and the host
 * re-runs the generic kernel, and group PRESENCE
 * is tracked in a per-thread bit mask so groups
 * whose sums are all zero still materialize. */
static void emit_body_baked(std::string &s, const Gen &G)
{
	s += "\tconstexpr int NG = " + std::to_string(G.nbake) + ";\n"
		"\tconstexpr long long GC[NG] = {";
	for (int q = 0; q < G.nbake; q++)
		s += fmt("%s%lldll", q ? ", " : "", G.bake[q]);
	s += "};\n";
	/* odd per-replica stride: spreads replicas across
	 * LDS banks (k_q1_agg's Q1_STRIDE trick) */
	s += "#define LPAD ((NG * LW * NA) | 1)\n";
	s += R"GG(
	__shared__ unsigned long long lvals[LREPL * LPAD];
	__shared__ unsigned int btouch;

	for (int q = threadIdx.x; q < LREPL * LPAD; q += blockDim.x)
		lvals[q] = 0;
	if (threadIdx.x == 0)
		btouch = 0;
	__syncthreads();
	const int lrep = (int) (threadIdx.x & (LREPL - 1));
	unsigned int tmask = 0;
	unsigned int nmiss = 0;
)GG";
	emit_loop_head(s, G);
	s += R"GG(		int g = -1;
#pragma unroll
		for (int q = 0; q < NG; q++)
			if (code == GC[q])
				g = q;
		if (g >= 0)
		{
			unsigned long long *mine = &lvals[lrep * LPAD];

			tmask |= 1u << g;
)GG";
	emit_transitions(s, G, "\t\t\t", DEST_BAKED);
	s += R"GG(		}
		else
			/* a code outside the baked set is impossible on
			 * re-execution over immutable tables; if it ever
			 * happens, flag it and let the host re-run the
			 * generic kernel (keeping the full global-table
			 * path INSIDE this loop cost ~35% extra
			 * instructions for a dead branch) */
			nmiss++;
	}
	if (nmiss)
		atomicOr(P.err, PL_ERR_BAKE_MISS);
	if (tmask)
		atomicOr(&btouch, tmask);
	__syncthreads();
	for (int q = threadIdx.x; q < NG; q += blockDim.x)
	{
		if (!((btouch >> q) & 1u))
			continue;
		int64_t slot = pl_slot(P, GC[q]);

		if (slot < 0) { atomicOr(P.err, PL_ERR_FULL); continue; }
)GG";
	emit_flushes(s, G, "lvals[rr * LPAD + (q * NA + %d) * LW]");
	s += "\t}\n";
}

static gg_status
compile_and_load(const std::string &src, int nbake,
		 std::shared_ptr<void> *out)
{
	const char *dump = getenv("GG_PLAN_RTC_DUMP");

	if (dump && dump[0])
	{
		FILE *f = fopen(dump, nbake > 0 ? "a" : "w");

		if (f)
		{
			fprintf(f, "/* ==== nbake=%d ==== */\n%s",
				nbake, src.c_str());
			fclose(f);
		}
	}
	hiprtcProgram prog;

	if (hiprtcCreateProgram(&prog, src.c_str(), "gg_plan.cu", 0, nullptr,
				nullptr) != HIPRTC_SUCCESS)
		return fail(GG_ENOTSUP, "hiprtcCreateProgram failed");
	const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
	hiprtcResult cr = hiprtcCompileProgram(prog, 3, opts);

	if (cr != HIPRTC_SUCCESS)
	{
		size_t ls = 0;

		hiprtcGetProgramLogSize(prog, &ls);
		std::string log(ls, 0);
		hiprtcGetProgramLog(prog, &log[0]);
		hiprtcDestroyProgram(&prog);
		return fail(GG_ENOTSUP, "plan rtc compile failed: %.300s",
			    log.c_str());
	}
	size_t csz = 0;

	hiprtcGetCodeSize(prog, &csz);
	std::vector<char> code(csz);
	hiprtcGetCode(prog, code.data());
	hiprtcDestroyProgram(&prog);

	auto rtc = std::make_shared<PlanRtc>();

	if (hipModuleLoadData(&rtc->mod, code.data()) != hipSuccess)
		return fail(GG_ENOTSUP, "plan rtc module load failed");
	if (hipModuleGetFunction(&rtc->fn, rtc->mod, "plan_kernel")
	    != hipSuccess)
		return fail(GG_ENOTSUP, "plan rtc function lookup failed");
	*out = rtc;
	return GG_OK;
}

/* generate + compile; returns GG_OK with *out set, or non-OK (caller
 * falls back to the interpreted kernel) */
gg_status
plan_rtc_compile(const PlanDev &D, bool has_gnull0, bool has_gnull1,
		 std::shared_ptr<void> *out, const long long *bake,
		 int nbake, bool fast, const PlanWhereDev *W,
		 const PlanGroupNDev *N)
{
	const char *dis = getenv("GG_PLAN_RTC");

	if (dis && dis[0] == '0')
		return fail(GG_ENOTSUP, "rtc disabled");
	if (nbake <= 0)
		fast = false;	/* the u64 fast tier exists only baked */

	/* NT loads: measured FLAT while the row loop carried the dead
	 * fallback (4.90 vs 4.96 ms, r02k) but +12% once the loop got
	 * lean (4.20 -> 3.76 ms, r02nt2) — same physics as k_q1_agg's
	 * +11%.  Default ON for baked kernels; GG_PLAN_RTC_NT=0 reverts. */
	const char *ntv = getenv("GG_PLAN_RTC_NT");
	bool nt = nbake > 0 && !(ntv && ntv[0] == '0');
	bool payload = false;

	for (int j = 0; j < D.njoins; j++)
		if (gg_join_builds_map(D.pl.jkind[j]))
			payload = true;
	Gen G{D, {has_gnull0, has_gnull1}, bake, nbake, fast, nt, payload, W,
	      N && N->k.n >= 3 ? N : nullptr};
	std::string s;

	emit_prelude(s, G);
	{
		/* waves/SIMD occupancy hint; 4 matches the hand kernels,
		 * sweepable (GG_PLAN_WAVES) — fewer waves = more VGPRs
		 * per wave for the register-heavy baked tier */
		int waves = 4;
		const char *wv = getenv("GG_PLAN_WAVES");

		if (wv && atoi(wv) >= 1 && atoi(wv) <= 8)
			waves = atoi(wv);
		s += fmt("extern \"C\" __global__ "
			 "__launch_bounds__(256, %d)\n"
			 "void plan_kernel(PlanDev P)\n{\n"
			 "\tconst int64_t stride = "
			 "(int64_t) gridDim.x * blockDim.x;\n"
			 /* NAGGS as a real constant for array bounds */
			 "\tconstexpr int NA = %d;\n", waves, D.naggs);
	}
	emit_row_pass(s, G);
	emit_agg_vals(s, G);
	if (D.ngroup == 0)
		emit_body_global(s, G);
	else if (nbake > 0)
		emit_body_baked(s, G);
	else
		emit_body_grouped(s, G);
	s += "}\n";
	return compile_and_load(s, nbake, out);
}

gg_status
plan_rtc_launch(hipStream_t s, const std::shared_ptr<void> &h,
		const PlanDev &P, int grid, int block, const PlanWhereDev *W,
		const PlanGroupNDev *N)
{
	PlanRtc *rtc = (PlanRtc *) h.get();
	size_t size = plan_arg_bytes(P, W, N);
	PlanDevGroupN A;

	/* the leading bytes are those of PlanDevWhere, and of PlanDev */
	A.p = P;
	if (W)
		A.wh = *W;
	else if (N)
		std::memset(&A.wh, 0, sizeof(A.wh));
	if (N)
		A.gn = *N;
	void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &A,
			  HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
			  HIP_LAUNCH_PARAM_END};

	GG_HIP(hipModuleLaunchKernel(rtc->fn, grid, 1, 1, block, 1, 1, 0, s,
				     nullptr, config));
	return GG_OK;
}

}				/* namespace gg */
