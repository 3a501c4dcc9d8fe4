/*
 * Generic compiled-plan kernels (engine_abi.h "generalized pipeline
 * descriptor"): ONE build kernel and ONE fused scan/filter/join/agg
 * kernel execute any descriptor-shaped query — no query-specific code.
 *
 * Reference semantics implemented:
 *   predicates    execScan.c:110–214 + execQual.c:6260 (conjunctive
 *                 range quals; NULL input → qual not true)
 *   semi joins    nodeHash.c:88 (build) / nodeHashjoin.c:78 (probe);
 *                 NULL join keys never match (nodeHash.c:1070–1077)
 *   inner joins   unique-keyed build side (PK–FK): the build maps key ->
 *                 build-row index, the scan gathers payload columns
 *                 (group keys, factors, chained probe keys) through it
 *                 (nodeHashjoin.c HJ_NEED_NEW_OUTER -> HJ_SCAN_BUCKET)
 *   left joins    the INNER map, where "no partner" NULL-extends the row
 *                 instead of dropping it (HJ_FILL_OUTER_TUPLE): every
 *                 column of that source then reads as NULL
 *   anti joins    the SEMI set with the test inverted (JOIN_ANTI, NOT
 *                 EXISTS): a NULL probe key matches nothing and survives
 *   group-by      execHHashagg.c:905 find-or-create; NULL keys group
 *                 together (:531)
 *   transitions   nodeAgg.c:413–460 strict rules: SUM/COUNT(col) skip
 *                 NULL inputs, COUNT(*) does not; MIN/MAX words
 *                 (int8smaller/int8larger) are order-encoded so both
 *                 combine by unsigned max with 0 as identity
 *                 (plan_dev.h PlanAggDev)
 *   agg filters   agg(...) FILTER (WHERE ...), the Aggref.aggfilter that
 *                 advance_aggregates (nodeAgg.c) evaluates ahead of the
 *                 strict transition: per-aggregate range conjunctions
 *                 over driving or payload columns, evaluated once per
 *                 surviving row; they never touch the groups
 *   where clauses engine_abi.h gg_plan_where: a qual in conjunctive normal
 *                 form (ExecEvalAnd over ExecEvalOr over atoms; ExecEvalNot
 *                 only inside the atoms), atoms being ranges, negated ranges,
 *                 column comparisons, IS [NOT] NULL (ExecEvalNullTest) and
 *                 IN-lists as equalities (ExecEvalScalarArrayOp).  An atom
 *                 is true or not true, a comparison over NULL not true;
 *                 ExecQual drops the row whose qual is not true
 *   agg exprs     products with (100±col) under numeric.c:1735 mul_var
 *                 scale addition (scaled-int exact arithmetic)
 *
 * Layouts: group table = open addressing, EMPTY = INT64_MIN bit
 * pattern; hash semi-set stores key ^ 0x8000…, 0 = empty (build keys
 * of INT64_MIN rejected at compile); dense build sides collapse to a
 * 1-bit membership bitmap under the same max(key) <= 8x rows guard as
 * the named pipelines.
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <array>
#include <cstdlib>
#include <utility>

#include "../../include/gg_pg_hash.h"
#include "engine_internal.h"

namespace gg
{

static constexpr int PL_THREADS = 256;
static constexpr int PL_MAX_BLOCKS = 2048;

/* the one grid clamp of the plan kernels, interpreted and generated
 * (plan.cpp sizes the hipRTC launches and the fast-tier proof by it) */
int pl_grid(int64_t n)
{
	int64_t b = (n + PL_THREADS - 1) / PL_THREADS;

	return (int) (b < 1 ? 1 : (b > PL_MAX_BLOCKS ? PL_MAX_BLOCKS : b));
}

template <int NT>
__device__ static inline int64_t pl_ld(const void *c, int w, int64_t i)
{
	if (NT)
		switch (w)
		{
			case 1:
				return __builtin_nontemporal_load(
					&((const uint8_t *) c)[i]);
			case 4:
				return __builtin_nontemporal_load(
					&((const int32_t *) c)[i]);
			default:
				return __builtin_nontemporal_load(
					&((const int64_t *) c)[i]);
		}
	switch (w)
	{
		case 1:
			return ((const uint8_t *) c)[i];
		case 4:
			return ((const int32_t *) c)[i];
		default:
			return ((const int64_t *) c)[i];
	}
}

template <int NT>
__device__ static inline bool
pl_preds_pass(const PlanPredDev *preds, int npreds, int64_t i)
{
	for (int p = 0; p < npreds; p++)
	{
		if (preds[p].nulls && preds[p].nulls[i])
			return false;	/* NULL comparison is not true */
		{
			int64_t v = pl_ld<NT>(preds[p].col, preds[p].width, i);

			if (v < preds[p].lo || v >= preds[p].hi)
				return false;
		}
	}
	return true;
}

/* 4 rows at once, predicate loads UNCONDITIONAL: short-circuiting per
 * row turns the scan into dependent sparse gathers (measured 2.3 TB/s
 * on Q6); streaming every predicate column and ANDing the results
 * keeps the loads wide and independent like the named pipelines. */
template <int NT>
__device__ static inline void
pl_preds_pass4(const PlanPredDev *preds, int npreds, int64_t i, int64_t S,
	       bool ok[4])
{
	ok[0] = ok[1] = ok[2] = ok[3] = true;
	for (int p = 0; p < npreds; p++)
	{
		const PlanPredDev &P = preds[p];
		int64_t v0 = pl_ld<NT>(P.col, P.width, i);
		int64_t v1 = pl_ld<NT>(P.col, P.width, i + S);
		int64_t v2 = pl_ld<NT>(P.col, P.width, i + 2 * S);
		int64_t v3 = pl_ld<NT>(P.col, P.width, i + 3 * S);

		ok[0] &= v0 >= P.lo && v0 < P.hi;
		ok[1] &= v1 >= P.lo && v1 < P.hi;
		ok[2] &= v2 >= P.lo && v2 < P.hi;
		ok[3] &= v3 >= P.lo && v3 < P.hi;
		if (P.nulls)
		{
			ok[0] &= !P.nulls[i];
			ok[1] &= !P.nulls[i + S];
			ok[2] &= !P.nulls[i + 2 * S];
			ok[3] &= !P.nulls[i + 3 * S];
		}
	}
}

/* ---- general WHERE clauses (engine_abi.h gg_plan_where) ---------------
 * One atom on loaded values: a, b the two columns widened to int64, na / nb
 * "the column is SQL NULL".  A comparison over a NULL is not true; IS_NULL
 * is true exactly then (ExecEvalNullTest).  True comparisons, never a
 * subtraction.  The kind is uniform over the wave, so the switch is a
 * scalar branch; the row's own work is branch-free. */
__device__ static inline bool
pl_atom_true(int kind, int64_t a, int64_t b, int64_t lo, int64_t hi, bool na,
	     bool nb)
{
	switch (kind)
	{
		case GG_ATOM_RANGE:
			return !na & (a >= lo) & (a < hi);
		case GG_ATOM_NOT_RANGE:
			return !na & ((a < lo) | (a >= hi));
		case GG_ATOM_LT:
			return !(na | nb) & (a < b);
		case GG_ATOM_LE:
			return !(na | nb) & (a <= b);
		case GG_ATOM_EQ:
			return !(na | nb) & (a == b);
		case GG_ATOM_NE:
			return !(na | nb) & (a != b);
		case GG_ATOM_IS_NULL:
			return na;
		default:	/* GG_ATOM_NOT_NULL */
			return !na;
	}
}

/* the scan clauses (every atom of source 0) of W at row i: OR within a
 * clause, AND across clauses (ExecEvalOr / ExecEvalAnd on true / not-true) */
__device__ static inline bool
pl_where_scan(const PlanWhereDev &W, int64_t i)
{
	bool ok = true;
	int q = 0;

	for (int c = 0; c < W.nscan; c++)
	{
		bool t = false;

		for (const int e = q + W.natoms[c]; q < e; q++)
		{
			const PlanAtomDev &A = W.atoms[q];
			int64_t a = 0, b = 0;
			bool nb = false;
			const bool na = A.nulls && A.nulls[i];

			if (A.kind < GG_ATOM_IS_NULL)
				a = pl_ld<0>(A.col, A.width, i);
			if (A.col2)
			{
				b = pl_ld<0>(A.col2, A.width2, i);
				nb = A.nulls2 && A.nulls2[i];
			}
			t |= pl_atom_true(A.kind, a, b, A.lo, A.hi, na, nb);
		}
		ok &= t;
	}
	return ok;
}

/* ... and for the 4 strided rows, under pl_preds_pass4's rule: every atom
 * column is loaded unconditionally for the four rows, no per-row short
 * circuit.  An atom over the column its predecessor in the clause read (an
 * IN-list) reuses the loaded values. */
__device__ static inline void
pl_where_scan4(const PlanWhereDev &W, int64_t i, int64_t S, bool ok[4])
{
	int q = 0;

	for (int c = 0; c < W.nscan; c++)
	{
		bool t[4] = {false, false, false, false};
		const void *last = nullptr;
		int64_t a[4] = {0, 0, 0, 0};
		bool na[4] = {false, false, false, false};

		for (const int e = q + W.natoms[c]; q < e; q++)
		{
			const PlanAtomDev &A = W.atoms[q];
			int64_t b[4] = {0, 0, 0, 0};
			bool nb[4] = {false, false, false, false};

			if (A.col != last)
			{
#pragma unroll
				for (int j = 0; j < 4; j++)
				{
					a[j] = pl_ld<0>(A.col, A.width, i + j * S);
					na[j] = A.nulls && A.nulls[i + j * S];
				}
				last = A.col;
			}
			if (A.col2)
#pragma unroll
				for (int j = 0; j < 4; j++)
				{
					b[j] = pl_ld<0>(A.col2, A.width2, i + j * S);
					nb[j] = A.nulls2 && A.nulls2[i + j * S];
				}
#pragma unroll
			for (int j = 0; j < 4; j++)
				t[j] |= pl_atom_true(A.kind, a[j], b[j], A.lo, A.hi,
						     na[j], nb[j]);
		}
#pragma unroll
		for (int j = 0; j < 4; j++)
			ok[j] &= t[j];
	}
}

/* ---- join build ------------------------------------------------------
 * INNER = 0: today's membership set (bitmap or hash set), duplicates
 * welcome.  INNER = 1: key -> build-row-index map for a unique-keyed
 * build side; a second passing row with the same non-NULL key sets
 * PL_ERR_DUP_KEY and the execute is refused.  The probe runs in a later
 * kernel, so the index write needs no ordering against the key CAS. */

template <int INNER>
__global__ __launch_bounds__(PL_THREADS, 4)
void k_plan_build(PlanBuildDev B)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < B.n; i += stride)
	{
		if (!pl_preds_pass<0>(B.preds, B.npreds, i))
			continue;
		/* scope 1+k clauses: a further filter of the build rows */
		if (B.wh.nscan && !pl_where_scan(B.wh, i))
			continue;
		if (B.knulls && B.knulls[i])
			continue;	/* NULL build key never matches */
		{
			int64_t k = pl_ld<0>(B.key, B.kw, i);

			if (INNER && B.dlen)
			{
				/* dense map: first row to claim the entry
				 * wins, a later one is a duplicate.  The
				 * sizing guard keeps every key inside the map
				 * (dlen = max + 1, and a negative key anywhere
				 * in the column forces the hash path); a key
				 * outside it would lose its partners, so it
				 * refuses the execute instead */
				if (k < 0 || k >= B.dlen ||
				    atomicCAS(&B.idx[k], PL_NOROW,
					      (uint32_t) i) != PL_NOROW)
					atomicOr(B.err, PL_ERR_DUP_KEY);
			}
			else if (B.bits)
			{
				if (k >= 0 && k < B.dlen)
					atomicOr(&B.bits[k >> 6],
						 1ull << (k & 63));
			}
			else
			{
				unsigned long long t = (unsigned long long) k
					^ PL_MSB;
				uint64_t pos = (uint64_t) gg_hashint8(k) &
					(B.hslots - 1);

				if (INNER && t == 0)
				{
					/* INT64_MIN encodes as the empty
					 * sentinel and could never be found */
					atomicOr(B.err, PL_ERR_DUP_KEY);
					continue;
				}
				for (uint64_t it = 0; it < B.hslots; it++)
				{
					unsigned long long cur =
						B.hkeys[pos];

					if (cur == t)
					{
						if (INNER)
							atomicOr(B.err,
								 PL_ERR_DUP_KEY);
						break;
					}
					if (cur == 0)
					{
						unsigned long long prev =
							atomicCAS(&B.hkeys[pos],
								  0ull, t);

						if (INNER && prev == 0)
							B.idx[pos] = (uint32_t) i;
						if (INNER && prev == t)
							atomicOr(B.err,
								 PL_ERR_DUP_KEY);
						if (prev == 0 || prev == t)
							break;
						continue;
					}
					pos = (pos + 1) & (B.hslots - 1);
				}
			}
		}
	}
}

hipError_t launch_plan_build(hipStream_t s, const PlanBuildDev &b)
{
	/* LEFT builds the INNER map, ANTI the SEMI set: the kinds differ in
	 * what the probe does with the answer, not in the structure */
	if (gg_join_builds_map(b.kind))
		hipLaunchKernelGGL(k_plan_build<1>, dim3(pl_grid(b.n)),
				   dim3(PL_THREADS), 0, s, b);
	else
		hipLaunchKernelGGL(k_plan_build<0>, dim3(pl_grid(b.n)),
				   dim3(PL_THREADS), 0, s, b);
	return hipGetLastError();
}

/* ---- fused scan + filter + semi-joins + group agg ------------------- */

__device__ static inline bool
pl_joins_pass(const PlanJoinDev *joins, int njoins, int64_t i)
{
	for (int j = 0; j < njoins; j++)
	{
		const PlanJoinDev &J = joins[j];

		if (J.pnulls && J.pnulls[i])
			return false;	/* NULL probe key never matches */
		{
			int64_t k = pl_ld<0>(J.pkey, J.width, i);

			if (J.bits)
			{
				if (k < 0 || k >= J.dlen ||
				    !((J.bits[k >> 6] >> (k & 63)) & 1))
					return false;
			}
			else
			{
				unsigned long long t = (unsigned long long) k
					^ PL_MSB;
				uint64_t pos = (uint64_t) gg_hashint8(k) &
					(J.hslots - 1);
				bool hit = false;

				for (;;)
				{
					unsigned long long cur =
						J.hkeys[pos];

					if (cur == t)
					{
						hit = true;
						break;
					}
					if (cur == 0)
						break;
					pos = (pos + 1) & (J.hslots - 1);
				}
				if (!hit)
					return false;
			}
		}
	}
	return true;
}

/* PL = the plan holds an INNER join: the row then carries the build-row
 * index of every INNER join, and a load of a column whose source is
 * 1+j indexes with join j's.  Plans without one instantiate PL = 0 and
 * compile to the code they always had (same treatment as MM below). */
template <int PL>
struct PlRow
{
};

template <>
struct PlRow<1>
{
	uint32_t r[GG_PLAN_MAX_JOINS];
};

/* PL = 2: the plan holds a LEFT or an ANTI join.  The row carries the same
 * indices, and r[j] == PL_NOROW says that LEFT join j found no partner:
 * the row is NULL-extended, every column of source 1+j reads as NULL.
 * That index must never reach a load (it is 0xFFFFFFFF and the build table
 * may have three rows): every consumer asks pl_src_null FIRST and takes
 * the NULL branch without computing an address.  Plans without such a
 * join stay on PL = 0 / 1 and compile to the code they always had. */
template <>
struct PlRow<2>
{
	uint32_t r[GG_PLAN_MAX_JOINS];
};

static_assert(GG_PLAN_MAX_JOINS == 2, "pl_ix selects between two joins");

/* source `src` is a LEFT join that NULL-extended this row */
template <int PL>
__device__ static inline bool
pl_src_null(const PlRow<PL> &R, int src)
{
	if constexpr (PL == 2)
		return src != 0 && (src == 1 ? R.r[0] : R.r[1]) == PL_NOROW;
	else
		return false;
}

template <int PL>
__device__ static inline int64_t
pl_ix(const PlRow<PL> &R, int src, int64_t i)
{
	if constexpr (PL)
		return src == 0 ? i : (int64_t) (src == 1 ? R.r[0] : R.r[1]);
	else
		return i;
}

/* A plan with scope-0 WHERE clauses: the kernel then gets them as one more
 * argument of its own, for the reason given at PlFilters below: no new
 * read of P.  The argument is a parameter pack, empty for a plan without
 * clauses, whose kernel so keeps its argument block to the byte and
 * compiles to the code it always had. */
struct PlWhere
{
	PlanWhereDev w;
};

__device__ static inline const PlanWhereDev &pl_where_arg(const PlWhere &W)
{
	return W.w;
}

/* A plan with three or four group columns (engine_abi.h gg_plan_groups).  It
 * is a fallback-tier plan like one with clauses and takes the same road: ONE
 * more instantiation, the most general one, whose extra argument carries the
 * clauses (none = a zeroed block, which passes every row) and, behind them,
 * the group block.  No new read of P, and no existing kernel's argument
 * block changes. */
struct PlWhereN
{
	PlanWhereDev w;
	PlanGroupNDev gn;
};

__device__ static inline const PlanWhereDev &pl_where_arg(const PlWhereN &W)
{
	return W.w;
}

__device__ static inline const PlanGroupNDev &pl_groupn_arg(const PlWhereN &W)
{
	return W.gn;
}

/* the post-join clauses of W, once per row that survived preds and joins.
 * Columns are read at the row their source names.  The test for a
 * NULL-extended source (pl_src_null, r == PL_NOROW) comes AHEAD of every
 * address computation, the NULL-flag load included: such a column is NULL
 * and neither its flag nor its value is loaded. */
template <int PL>
__device__ static inline bool
pl_where_post(const PlanWhereDev &W, int64_t i, const PlRow<PL> &R)
{
	int q = 0;

	for (int c = 0; c < W.nscan; c++)
		q += W.natoms[c];
	for (int c = W.nscan; c < W.nclauses; c++)
	{
		bool t = false;

		for (const int e = q + W.natoms[c]; q < e; q++)
		{
			const PlanAtomDev &A = W.atoms[q];
			int64_t a = 0, b = 0;
			bool na = true, nb = false;

			if (!pl_src_null<PL>(R, A.src))
			{
				const int64_t ia = pl_ix<PL>(R, A.src, i);

				na = A.nulls && A.nulls[ia];
				if (A.kind < GG_ATOM_IS_NULL)
					a = pl_ld<0>(A.col, A.width, ia);
			}
			if (A.col2)
			{
				nb = true;
				if (!pl_src_null<PL>(R, A.src2))
				{
					const int64_t ib = pl_ix<PL>(R, A.src2, i);

					nb = A.nulls2 && A.nulls2[ib];
					b = pl_ld<0>(A.col2, A.width2, ib);
				}
			}
			t |= pl_atom_true(A.kind, a, b, A.lo, A.hi, na, nb);
		}
		if (!t)
			return false;
	}
	return true;
}

/* the same walk for a plan with an INNER join: joins run in descriptor
 * order, an INNER join leaves its build-row index in R, and a probe key
 * may itself come from an earlier INNER join's build row */
__device__ static inline bool
pl_joins_index(const PlanDev &P, int64_t i, PlRow<1> &R)
{
	const PlanJoinDev *joins = P.joins;
	const int njoins = P.njoins;

	R.r[0] = R.r[1] = 0;
#pragma unroll
	for (int j = 0; j < GG_PLAN_MAX_JOINS; j++)
	{
		if (j >= njoins)
			break;
		const PlanJoinDev &J = joins[j];
		const bool inner = P.pl.jkind[j] == GG_JOIN_INNER;
		int64_t pi = pl_ix<1>(R, P.pl.jpsrc[j], i);

		if (J.pnulls && J.pnulls[pi])
			return false;	/* NULL probe key never matches */
		int64_t k = pl_ld<0>(J.pkey, J.width, pi);

		if (inner && J.dlen)
		{
			/* range check BEFORE the map is touched */
			if (k < 0 || k >= J.dlen)
				return false;
			uint32_t x = P.pl.jidx[j][k];

			if (x == PL_NOROW)
				return false;
			R.r[j] = x;
		}
		else if (inner)
		{
			unsigned long long t = (unsigned long long) k
				^ PL_MSB;
			uint64_t pos = (uint64_t) gg_hashint8(k) &
				(J.hslots - 1);

			/* empty BEFORE match: a probe key of INT64_MIN
			 * encodes as the empty sentinel and must not "hit"
			 * a slot whose index was never written */
			for (;;)
			{
				unsigned long long cur = J.hkeys[pos];

				if (cur == 0)
					return false;
				if (cur == t)
					break;
				pos = (pos + 1) & (J.hslots - 1);
			}
			R.r[j] = P.pl.jidx[j][pos];
		}
		else if (J.bits)
		{
			if (k < 0 || k >= J.dlen ||
			    !((J.bits[k >> 6] >> (k & 63)) & 1))
				return false;
		}
		else
		{
			/* SEMI hash set, probed as pl_joins_pass does */
			unsigned long long t = (unsigned long long) k
				^ PL_MSB;
			uint64_t pos = (uint64_t) gg_hashint8(k) &
				(J.hslots - 1);

			for (;;)
			{
				unsigned long long cur = J.hkeys[pos];

				if (cur == t)
					break;
				if (cur == 0)
					return false;
				pos = (pos + 1) & (J.hslots - 1);
			}
		}
	}
	return true;
}

/* ... and for a plan with a LEFT or an ANTI join (engine_abi.h
 * gg_plan_join; nodeHashjoin.c HJ_FILL_OUTER_TUPLE / JOIN_ANTI).  One
 * probe per join yields "has a partner" (and, for the two map kinds, its
 * build row); the kind then decides: SEMI and INNER drop the row without
 * one, ANTI drops the row WITH one, LEFT keeps every row and leaves
 * PL_NOROW where there is none.  A NULL probe key matches nothing
 * (nodeHash.c:1070) and is never probed; a probe key whose source is a
 * NULL-extended LEFT join is NULL, and neither its flag nor its value is
 * loaded. */
__device__ static inline bool
pl_joins_outer(const PlanDev &P, int64_t i, PlRow<2> &R)
{
	const int njoins = P.njoins;

	R.r[0] = R.r[1] = 0;
#pragma unroll
	for (int j = 0; j < GG_PLAN_MAX_JOINS; j++)
	{
		if (j >= njoins)
			break;
		const PlanJoinDev &J = P.joins[j];
		const int kind = P.pl.jkind[j];
		const bool map = kind == GG_JOIN_INNER || kind == GG_JOIN_LEFT;
		const int psrc = P.pl.jpsrc[j];
		bool hit = false;
		uint32_t x = PL_NOROW;

		if (!pl_src_null<2>(R, psrc))
		{
			const int64_t pi = pl_ix<2>(R, psrc, i);

			if (!(J.pnulls && J.pnulls[pi]))
			{
				const int64_t k = pl_ld<0>(J.pkey, J.width, pi);

				if (map && J.dlen)
				{
					/* range check BEFORE the map is touched: a
					 * key outside it has no partner */
					if (k >= 0 && k < J.dlen)
					{
						x = P.pl.jidx[j][k];
						hit = x != PL_NOROW;
					}
				}
				else if (J.bits)
				{
					hit = k >= 0 && k < J.dlen &&
						((J.bits[k >> 6] >> (k & 63)) & 1);
				}
				else
				{
					/* key -> index map, SEMI or ANTI set.
					 * Empty BEFORE match for the map and for
					 * ANTI: a probe key of INT64_MIN encodes
					 * as the empty sentinel, is in no set and
					 * must not read an unwritten index; SEMI
					 * keeps the order pl_joins_pass has */
					const unsigned long long t =
						(unsigned long long) k ^
						PL_MSB;
					uint64_t pos = (uint64_t) gg_hashint8(k) &
						(J.hslots - 1);
					const bool semi = kind == GG_JOIN_SEMI;

					for (;;)
					{
						unsigned long long cur = J.hkeys[pos];

						if (cur == 0 && !semi)
							break;
						if (cur == t)
						{
							hit = true;
							break;
						}
						if (cur == 0)
							break;
						pos = (pos + 1) & (J.hslots - 1);
					}
					if (hit && map)
						x = P.pl.jidx[j][pos];
				}
			}
		}
		if (kind == GG_JOIN_LEFT)
			R.r[j] = hit ? x : PL_NOROW;
		else if (kind == GG_JOIN_ANTI)
		{
			if (hit)
				return false;
		}
		else
		{
			if (!hit)
				return false;
			if (map)
				R.r[j] = x;
		}
	}
	return true;
}

template <int PL>
__device__ static inline bool
pl_row_joins(const PlanDev &P, int64_t i, PlRow<PL> &R)
{
	if constexpr (PL == 2)
		return pl_joins_outer(P, i, R);
	else if constexpr (PL)
		return pl_joins_index(P, i, R);
	else
		return pl_joins_pass(P.joins, P.njoins, i);
}

/* group code; INT64_MIN bit pattern = empty sentinel (never a code).
 * GP = the plan groups by a packed pair (PlanGroupPackDev); every other
 * plan instantiates GP = 0 and compiles to the code it always had. */
template <int PL, int GP>
__device__ static inline long long
pl_group_code(const PlanDev &P, int64_t i, const PlRow<PL> &R)
{
	if (P.ngroup == 0)
		return 0;
	const int64_t i0 = pl_ix<PL>(R, P.pl.gsrc[0], i);

	if constexpr (GP)
	{
		/* e = 0 for NULL, else v - min + 1, in unsigned arithmetic
		 * (the difference is below 2^62, the operands need not be);
		 * the widths sum to <= 62, so the code is non-negative */
		const int64_t i1 = pl_ix<PL>(R, P.pl.gsrc[1], i);
		unsigned long long e0 = (pl_src_null<PL>(R, P.pl.gsrc[0]) ||
					 (P.gnulls[0] && P.gnulls[0][i0])) ? 0ull
			: (unsigned long long) pl_ld<0>(P.gcol[0], P.gwidth[0], i0)
			- (unsigned long long) P.gp.gmin[0] + 1ull;
		unsigned long long e1 = (pl_src_null<PL>(R, P.pl.gsrc[1]) ||
					 (P.gnulls[1] && P.gnulls[1][i1])) ? 0ull
			: (unsigned long long) pl_ld<0>(P.gcol[1], P.gwidth[1], i1)
			- (unsigned long long) P.gp.gmin[1] + 1ull;

		return (long long) ((e0 << P.gp.shift) | e1);
	}
	if (P.ngroup == 2)
	{
		/* two char1 columns; NULL encodes as 256 so NULL groups
		 * stay distinct per column (execHHashagg.c:531) */
		const int64_t i1 = pl_ix<PL>(R, P.pl.gsrc[1], i);
		long long e0 = (pl_src_null<PL>(R, P.pl.gsrc[0]) ||
				(P.gnulls[0] && P.gnulls[0][i0])) ? 256
			: pl_ld<0>(P.gcol[0], P.gwidth[0], i0);
		long long e1 = (pl_src_null<PL>(R, P.pl.gsrc[1]) ||
				(P.gnulls[1] && P.gnulls[1][i1])) ? 256
			: pl_ld<0>(P.gcol[1], P.gwidth[1], i1);

		return e0 * 512 + e1;
	}
	if (pl_src_null<PL>(R, P.pl.gsrc[0]) ||
	    (P.gnulls[0] && P.gnulls[0][i0]))
		return GG_PLAN_NULL_KEY;
	return pl_ld<0>(P.gcol[0], P.gwidth[0], i0);
}

/* GP = 2: the code of G = N.k.n >= 3 packed fields (plan_dev.h PlanKeysN),
 * field g = e_g << shift[g], e_g as in the packed pair and in the same
 * unsigned arithmetic; the widths sum to <= 62, so the code is non-negative.
 * Columns 0 and 1 are P's, columns 2 and 3 the block's. */
template <int PL>
__device__ static inline long long
pl_group_code_n(const PlanDev &P, const PlanGroupNDev &N, int64_t i,
		const PlRow<PL> &R)
{
	unsigned long long code = 0;

	for (int g = 0; g < N.k.n && g < PL_MAX_GCOLS; g++)
	{
		const PlanGroupCol C = plan_group_col(P, N, g);
		unsigned long long e = 0;

		/* the NULL-extended source is tested ahead of every address
		 * computation, the flag load included */
		if (!pl_src_null<PL>(R, C.src))
		{
			const int64_t ig = pl_ix<PL>(R, C.src, i);

			if (!(C.nulls && C.nulls[ig]))
				e = (unsigned long long) pl_ld<0>(C.col, C.width, ig)
					- (unsigned long long) N.k.gmin[g] + 1ull;
		}
		code |= e << N.k.shift[g];
	}
	return (long long) code;
}

/* strict-transition aggregate input (nodeAgg.c:413).  MM = the plan
 * holds a MIN/MAX word: plans without one instantiate the kernel with
 * MM = 0 and carry none of the kind >= 3 branches (the interpreted
 * Q1-shaped plan measured 2.6% slower with them in the row loop). */
template <int MM, int PL>
__device__ static inline bool
pl_agg_val(const PlanAggDev &a, const int8_t *src, int64_t i,
	   const PlRow<PL> &R, __int128 *out)
{
	if (a.kind == 0)	/* COUNT(*) */
	{
		*out = 1;
		return true;
	}
	for (int f = 0; f < a.nf; f++)
		if (pl_src_null<PL>(R, src[f]) ||
		    (a.nulls[f] && a.nulls[f][pl_ix<PL>(R, src[f], i)]))
			return false;	/* strict: skip NULL input */
	if (a.kind == 1)	/* COUNT(col) */
	{
		*out = 1;
		return true;
	}
	{
		__int128 v = 1;

		for (int f = 0; f < a.nf; f++)
		{
			int64_t x = pl_ld<0>(a.col[f], a.width[f],
					     pl_ix<PL>(R, src[f], i));

			if (a.mod[f] == 1)
				x = 100 - x;
			else if (a.mod[f] == 2)
				x = 100 + x;
			v *= x;
		}
		if (MM && a.kind >= 3)	/* MIN / MAX word: one factor, encoded
					 * AFTER the modifier */
		{
			unsigned long long e = (unsigned long long) v ^
				PL_MSB;

			v = (__int128) (a.kind == 3 ? ~e : e);
		}
		*out = v;
		return true;
	}
}

/* FL = some aggregate carries a filter.  The kernel then gets the plan's
 * PlanFilterDev as a kernel argument of its own and reads nothing of
 * P.fl: every read of P counts against the compiler's limit (300 users)
 * for serving a by-value argument straight from the kernarg segment, the
 * PL = 1 kernels sit close to it, and past it the whole of P is copied to
 * scratch and every column load turns flat (seen in the ISA: 2000 bytes
 * of scratch, no global_load left).  Plans without a filter instantiate
 * FL = 0, carry an empty argument, and compile to the code they always
 * had. */
template <int FL>
struct PlFilters
{
};

template <>
struct PlFilters<1>
{
	PlanFilterDev f;
};

/* aggregate filters: every referenced filter once per surviving row, NULL
 * flag first, into a bitmask (bit k = filter k is true).  Columns are
 * read at the row their source names, so a payload predicate sees the
 * joined build row. */
template <int PL>
__device__ static inline unsigned
pl_row_filters(const PlanFilterDev &F, int64_t i, const PlRow<PL> &R)
{
	unsigned fm = 0;

#pragma unroll
	for (int k = 0; k < GG_PLAN_MAX_FILTERS; k++)
	{
		if (!((F.used >> k) & 1))
			continue;
		bool ok = true;

		for (int q = 0; ok && q < F.npreds[k]; q++)
		{
			const PlanPredDev &C = F.preds[k][q];
			const int64_t fi = pl_ix<PL>(R, F.psrc[k][q], i);

			if (pl_src_null<PL>(R, F.psrc[k][q]) ||
			    (C.nulls && C.nulls[fi]))
				ok = false;	/* NULL comparison is not true */
			else
			{
				int64_t v = pl_ld<0>(C.col, C.width, fi);

				ok = v >= C.lo && v < C.hi;
			}
		}
		if (ok)
			fm |= 1u << k;
	}
	return fm;
}

/* one row's transitions: every aggregate's value into its two-word
 * accumulator acc(a).  ATOMIC = the accumulators live in LDS
 * or global memory, else in registers.  Exact 128-bit add, or unsigned
 * max of the encoded MIN/MAX word.  FL = the plan references an
 * aggregate filter: fm holds the row's filter bits and an aggregate whose
 * filter bit is clear skips the row, ahead of everything else (COUNT(*)
 * included).  Plans without one instantiate FL = 0 and compile to the
 * code they always had. */
template <int MM, int PL, int FL, bool ATOMIC, class Acc>
__device__ static inline void
pl_row_aggs(const PlanDev &P, const PlFilters<FL> &F, int64_t i,
	    const PlRow<PL> &R, unsigned fm, Acc acc)
{
	for (int a = 0; a < P.naggs; a++)
	{
		__int128 v;

		if constexpr (FL)
		{
			const int f = F.f.afilt[a];

			if (f && !((fm >> (f - 1)) & 1))
				continue;
		}
		if (!pl_agg_val<MM, PL>(P.aggs[a], P.pl.asrc[a], i, R, &v))
			continue;
		unsigned long long vlo = (unsigned long long) v;
		unsigned long long vhi = (unsigned long long) (v >> 64);
		unsigned long long *w = acc(a);

		if (MM && P.aggs[a].kind >= 3)
		{
			if (ATOMIC)
				atomicMax(w, vlo);
			else if (vlo > w[0])
				w[0] = vlo;
		}
		else if (ATOMIC)
			pl_atomic_add128(w, vlo, vhi);
		else
			pl_add128(w[0], w[1], vlo, vhi);
	}
}

/* fold the replicas of accumulator a (replica rr's words at rep(rr))
 * and flush the result into the global accumulator dst */
template <int MM, int NREP, class Rep>
__device__ static inline void
pl_fold_flush(int kind, unsigned long long *dst, Rep rep)
{
	unsigned long long lo = 0, hi = 0;

	if (MM && kind >= 3)
	{
		for (int rr = 0; rr < NREP; rr++)
			if (rep(rr)[0] > lo)
				lo = rep(rr)[0];
		if (lo)
			atomicMax(dst, lo);
		return;
	}
	for (int rr = 0; rr < NREP; rr++)
		pl_add128(lo, hi, rep(rr)[0], rep(rr)[1]);
	if (lo || hi)
		pl_atomic_add128(dst, lo, hi);
}

template <int NT, int MM, int PL, int GP, int FL, class... Where>
__global__ __launch_bounds__(PL_THREADS, 4)
void k_plan_scan_agg(PlanDev P, PlFilters<FL> F, Where... W)
{
	constexpr bool WH = sizeof...(Where) != 0;

	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	/* Both group modes scan the same way: 4-way strided rows with
	 * unconditional predicate streams, then the tail.  The loop is
	 * spelled out per mode on purpose: shared through a lambda or a
	 * template it is optimized before the row body is inlined and the
	 * whole kernel compiles differently (4789 instead of 5960
	 * instructions), which this kernel's measured speed never saw. */
	if (P.ngroup == 0)
	{
		/* global-group fast path: register accumulators, one
		 * wave-reduced atomic flush per wave (the Q1/sumprice
		 * pattern — keeps e.g. Q6 at streaming rate) */
		unsigned long long acc[GG_PLAN_MAX_AGGS][2] = {};
		auto row = [&](int64_t i)
		{
			PlRow<PL> R;

			if (!pl_row_joins<PL>(P, i, R))
				return;
			if constexpr (WH)
				if (!pl_where_post<PL>(pl_where_arg(W...), i, R))
					return;
			unsigned fm = 0;

			if constexpr (FL)
				fm = pl_row_filters<PL>(F.f, i, R);
			pl_row_aggs<MM, PL, FL, false>(P, F, i, R, fm,
						       [&](int a) { return acc[a]; });
		};
		int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;

		for (; i + 3 * stride < P.n; i += 4 * stride)
		{
			bool ok[4];

			pl_preds_pass4<NT>(P.preds, P.npreds, i, stride, ok);
			if constexpr (WH)
				pl_where_scan4(pl_where_arg(W...), i, stride, ok);
			for (int j = 0; j < 4; j++)
				if (ok[j])
					row(i + j * stride);
		}
		for (; i < P.n; i += stride)
		{
			if constexpr (WH)
				if (!pl_where_scan(pl_where_arg(W...), i))
					continue;
			if (pl_preds_pass<NT>(P.preds, P.npreds, i))
				row(i);
		}
		for (int a = 0; a < P.naggs; a++)
		{
			if (MM && P.aggs[a].kind >= 3)
			{
				/* encoded MIN/MAX word: wave max, then one
				 * global max per wave; 0 = no input seen */
				for (int off = 32; off; off >>= 1)
				{
					unsigned long long o =
						__shfl_down(acc[a][0], off, 64);

					if (o > acc[a][0])
						acc[a][0] = o;
				}
				if ((threadIdx.x & 63) == 0 && acc[a][0])
					atomicMax(&P.tvals[2 * a], acc[a][0]);
				continue;
			}
			for (int off = 32; off; off >>= 1)
				pl_add128(acc[a][0], acc[a][1],
					  __shfl_down(acc[a][0], off, 64),
					  __shfl_down(acc[a][1], off, 64));
			if ((threadIdx.x & 63) == 0 && (acc[a][0] || acc[a][1]))
				pl_atomic_add128(&P.tvals[2 * a], acc[a][0],
						 acc[a][1]);
		}
		/* mark slot 0 used so compaction emits the group */
		if (blockIdx.x == 0 && threadIdx.x == 0)
			P.tkeys[0] = 0;
		return;
	}

	/* Per-block LDS group cache: low-cardinality group-bys (Q1's 6
	 * groups, nation's 25) otherwise hammer a handful of global
	 * accumulator words with per-row atomics — the ~88 atomics/µs
	 * hot-word wall.  64-slot LDS open addressing absorbs the per-row
	 * transitions; overflow rows (cardinality > ~64 per block) fall
	 * back to the global table, and the LDS slots flush once per
	 * block (execHHashagg.c:456 find-or-create, two-level). */
	constexpr int LSLOTS = 32;
	constexpr int LREPL = 8;	/* replicas split the per-word LDS
					 * atomic serialization 8 ways (the
					 * k_q1_agg replica pattern) */
	constexpr long long LEMPTY = (long long) PL_EMPTY;
	__shared__ long long lkeys[LSLOTS];
	__shared__ unsigned long long
		lvals[LREPL][LSLOTS][2 * GG_PLAN_MAX_AGGS];

	for (int s = threadIdx.x; s < LSLOTS; s += blockDim.x)
		lkeys[s] = LEMPTY;
	for (int s = threadIdx.x;
	     s < LREPL * LSLOTS * 2 * GG_PLAN_MAX_AGGS; s += blockDim.x)
		((unsigned long long *) lvals)[s] = 0;
	__syncthreads();

	const int lrep = (int) (threadIdx.x & (LREPL - 1));

	auto row = [&](int64_t i)
	{
		PlRow<PL> R;

		if (!pl_row_joins<PL>(P, i, R))
			return;
		if constexpr (WH)
			if (!pl_where_post<PL>(pl_where_arg(W...), i, R))
				return;
		unsigned fm = 0;

		if constexpr (FL)
			fm = pl_row_filters<PL>(F.f, i, R);
		long long code;

		if constexpr (GP == 2)
			code = pl_group_code_n<PL>(P, pl_groupn_arg(W...), i, R);
		else
			code = pl_group_code<PL, GP>(P, i, R);
		int ls = -1;
		uint32_t pos = (uint32_t) gg_hashint8(code) & (LSLOTS - 1);

		for (int probe = 0; probe < 8; probe++)
		{
			long long cur = lkeys[pos];

			if (cur == code)
			{
				ls = (int) pos;
				break;
			}
			if (cur == LEMPTY)
			{
				long long prev = atomicCAS(
					(unsigned long long *) &lkeys[pos],
					(unsigned long long) LEMPTY,
					(unsigned long long) code);

				if (prev == LEMPTY || prev == code)
				{
					ls = (int) pos;
					break;
				}
				continue;
			}
			pos = (pos + 1) & (LSLOTS - 1);
		}
		if (ls >= 0)
		{
			pl_row_aggs<MM, PL, FL, true>(P, F, i, R, fm, [&](int a)
			{
				return &lvals[lrep][ls][2 * a];
			});
			return;
		}
		/* cache full: straight into the global table */
		int64_t slot = pl_slot(P, code);

		if (slot < 0)
		{
			atomicOr(P.err, PL_ERR_FULL);
			return;
		}
		pl_row_aggs<MM, PL, FL, true>(P, F, i, R, fm, [&](int a)
		{
			return &P.tvals[(slot * P.naggs + a) * 2];
		});
	};
	int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;

	for (; i + 3 * stride < P.n; i += 4 * stride)
	{
		bool ok[4];

		pl_preds_pass4<NT>(P.preds, P.npreds, i, stride, ok);
		if constexpr (WH)
			pl_where_scan4(pl_where_arg(W...), i, stride, ok);
		for (int j = 0; j < 4; j++)
			if (ok[j])
				row(i + j * stride);
	}
	for (; i < P.n; i += stride)
	{
		if constexpr (WH)
			if (!pl_where_scan(pl_where_arg(W...), i))
				continue;
		if (pl_preds_pass<NT>(P.preds, P.npreds, i))
			row(i);
	}

	/* flush the block's LDS groups into the global table */
	__syncthreads();
	for (int s = threadIdx.x; s < LSLOTS; s += blockDim.x)
	{
		if (lkeys[s] == LEMPTY)
			continue;
		int64_t slot = pl_slot(P, lkeys[s]);

		if (slot < 0)
		{
			atomicOr(P.err, PL_ERR_FULL);
			continue;
		}
		for (int a = 0; a < P.naggs; a++)
			pl_fold_flush<MM, LREPL>(
				P.aggs[a].kind,
				&P.tvals[(slot * P.naggs + a) * 2],
				[&](int rr) { return &lvals[rr][s][2 * a]; });
	}
}

template <int FL>
static PlFilters<FL> pl_filters_arg(const PlanDev &p)
{
	PlFilters<FL> F;

	if constexpr (FL)
		F.f = p.fl;
	return F;
}

/* The host launcher of one k_plan_scan_agg instantiation, and the table of
 * all 48.  Entry i holds the flags pl_decode(i) gives: PL in {0, 1, 2} is
 * the lowest digit, above it one bit each for MM, NT, GP and FL.  The table
 * is built from the index sequence alone, and pl_encode is the inverse
 * launch_plan_scan_agg indexes it by; the static_asserts below pin the pair
 * at every flag, so a wrong mapping fails the build. */
template <int NT, int MM, int PL, int GP, int FL>
static void pl_launch(hipStream_t s, const PlanDev &p)
{
	hipLaunchKernelGGL((k_plan_scan_agg<NT, MM, PL, GP, FL>),
			   dim3(pl_grid(p.n)), dim3(PL_THREADS), 0, s, p,
			   pl_filters_arg<FL>(p));
}

/* A plan with scope-0 WHERE clauses.  The interpreted kernel is the
 * fallback tier (such a plan normally runs its generated kernel), so the
 * clauses buy two instantiations, not another 48: they imply NT = 0 and
 * the most general value of every flag whose general form also serves the
 * plans of the lesser ones: MM = 1 (the MIN/MAX branches are behind the
 * accumulator's kind), PL = 2 (pl_joins_outer walks all four join kinds and
 * none) and FL = 1 (an empty `used` mask evaluates nothing).  GP stays a
 * flag: the packed code is not a superset of the others. */
static_assert(sizeof(PlanDev) + sizeof(PlFilters<1>) + sizeof(PlWhereN) <=
	      4096 && sizeof(PlWhereN) >= sizeof(PlWhere),
	      "the interpreted kernel's arguments fit a kernarg segment");

template <int GP>
static void pl_launch_where(hipStream_t s, const PlanDev &p,
			    const PlanWhereDev &w)
{
	PlWhere W;

	W.w = w;
	hipLaunchKernelGGL((k_plan_scan_agg<0, 1, 2, GP, 1, PlWhere>),
			   dim3(pl_grid(p.n)), dim3(PL_THREADS), 0, s, p,
			   pl_filters_arg<1>(p), W);
}

/* ... and a plan with three or four group columns, with or without clauses:
 * GP = 2 on the same general flags (see PlWhereN) */
static void pl_launch_groupn(hipStream_t s, const PlanDev &p,
			     const PlanWhereDev *w, const PlanGroupNDev &gn)
{
	PlWhereN W = {};

	if (w)
		W.w = *w;
	W.gn = gn;
	hipLaunchKernelGGL((k_plan_scan_agg<0, 1, 2, 2, 1, PlWhereN>),
			   dim3(pl_grid(p.n)), dim3(PL_THREADS), 0, s, p,
			   pl_filters_arg<1>(p), W);
}

typedef void (*PlLaunchFn)(hipStream_t, const PlanDev &);
struct PlFlags
{
	int nt, mm, pl, gp, fl;
};
static constexpr int PL_NKERNELS = 2 * 2 * 3 * 2 * 2;

static constexpr PlFlags pl_decode(int i)
{
	return {i / 6 % 2, i / 3 % 2, i % 3, i / 12 % 2, i / 24};
}

static constexpr int pl_encode(bool nt, bool mm, int pl, bool gp, bool fl)
{
	return pl + 3 * (mm + 2 * (nt + 2 * (gp + 2 * fl)));
}

template <int... I>
static constexpr std::array<PlLaunchFn, sizeof...(I)>
pl_table(std::integer_sequence<int, I...>)
{
	return {{&pl_launch<pl_decode(I).nt, pl_decode(I).mm, pl_decode(I).pl,
			    pl_decode(I).gp, pl_decode(I).fl>...}};
}

static constexpr auto PL_TABLE =
	pl_table(std::make_integer_sequence<int, PL_NKERNELS>{});

/* the entry pl_encode names for these flags launches exactly their kernel */
template <int NT, int MM, int PL, int GP, int FL>
static constexpr bool pl_pinned()
{
	return PL_TABLE[pl_encode(NT, MM, PL, GP, FL)] ==
		&pl_launch<NT, MM, PL, GP, FL>;
}

static_assert(pl_pinned<0, 0, 0, 0, 0>() && pl_pinned<1, 1, 2, 1, 1>() &&
	      pl_encode(1, 1, 2, 1, 1) == PL_NKERNELS - 1 &&
	      pl_pinned<1, 0, 0, 0, 0>() && pl_pinned<0, 1, 0, 0, 0>() &&
	      pl_pinned<0, 0, 1, 0, 0>() && pl_pinned<0, 0, 2, 0, 0>() &&
	      pl_pinned<0, 0, 0, 1, 0>() && pl_pinned<0, 0, 0, 0, 1>(),
	      "k_plan_scan_agg launcher table: decode and encode disagree");

hipError_t launch_plan_scan_agg(hipStream_t s, const PlanDev &p,
				const PlanWhereDev *w, const PlanGroupNDev *gn)
{
	if (gn)
	{
		pl_launch_groupn(s, p, w, *gn);
		return hipGetLastError();
	}
	if (w)
	{
		if (p.ngroup == 2 && p.gp.packed)
			pl_launch_where<1>(s, p, *w);
		else
			pl_launch_where<0>(s, p, *w);
		return hipGetLastError();
	}

	const char *nt = getenv("GG_PLAN_NT");
	bool mm = false;
	/* 1: the row carries build-row indices (an INNER join); 2: a LEFT or
	 * ANTI join anywhere, the kernels that walk all four join kinds (an
	 * ANTI-only plan rides along, so pl_joins_pass stays what it was).
	 * 2 wins over 1 */
	int pl = 0;

	for (int a = 0; a < p.naggs; a++)
		if (p.aggs[a].kind >= 3)
			mm = true;
	for (int j = 0; j < p.njoins; j++)
		pl = std::max(pl, gg_join_keeps_unmatched(p.pl.jkind[j]) ? 2
			      : gg_join_builds_map(p.pl.jkind[j]) ? 1 : 0);
	PL_TABLE[pl_encode(nt && nt[0] == '1', mm, pl,
			   /* a packed pair of group columns */
			   p.ngroup == 2 && p.gp.packed,
			   /* some aggregate carries a filter */
			   p.fl.used != 0)](s, p);
	return hipGetLastError();
}

/* compact used slots into rows of (code, naggs x (lo,hi)) */
__global__ __launch_bounds__(PL_THREADS, 4)
void k_plan_compact(const unsigned long long *__restrict__ tkeys,
		    const unsigned long long *__restrict__ tvals,
		    uint64_t nslots, int naggs,
		    unsigned long long *__restrict__ out,
		    unsigned long long *out_n, uint64_t cap)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	const int rowsz = 1 + 2 * naggs;

	for (int64_t s = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     s < (int64_t) nslots; s += stride)
	{
		unsigned long long k = tkeys[s];
		bool take = k != PL_EMPTY;
		unsigned long long mask = __ballot(take);
		int lane = (int) (threadIdx.x & 63);
		unsigned long long base = 0;

		if (mask)
		{
			int leader = __ffsll((long long) mask) - 1;

			if (lane == leader)
				base = atomicAdd(out_n,
						 (unsigned long long)
						 __popcll(mask));
			base = __shfl(base, leader, 64);
		}
		if (!take)
			continue;
		{
			unsigned long long idx = base +
				(unsigned long long) __popcll(
					mask & ((1ull << lane) - 1));

			if (idx >= cap)
				continue;
			{
				unsigned long long *row = out + idx * rowsz;

				row[0] = k;
				for (int a = 0; a < 2 * naggs; a++)
					row[1 + a] =
						tvals[s * 2 * naggs + a];
			}
		}
	}
}

hipError_t launch_plan_compact(hipStream_t s,
			       const unsigned long long *tkeys,
			       const unsigned long long *tvals,
			       uint64_t nslots, int naggs,
			       unsigned long long *out,
			       unsigned long long *out_n, uint64_t cap)
{
	hipLaunchKernelGGL(k_plan_compact, dim3(pl_grid((int64_t) nslots)),
			   dim3(PL_THREADS), 0, s, tkeys, tvals, nslots,
			   naggs, out, out_n, cap);
	return hipGetLastError();
}

}				/* namespace gg */
