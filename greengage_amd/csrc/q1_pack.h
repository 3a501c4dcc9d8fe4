/*
 * Host-side arithmetic of the packed Q1 companion ("Packed Q1
 * companion"): which tables may be narrowed, how many blocks the packed
 * scan needs so that a block's u64 partial sums cannot wrap, and the
 * cutoff in the 16-bit shipdate domain.  Plain functions with no HIP
 * dependency: engine_abi.cpp and kernels.hip use them, and
 * tests/test_q1_pack_cpu.py compiles them into a stand-alone program.
 *
 * Layout, one entry per row:
 *   w8 (u64): price bits 0-31 | qty 32-47 | disc 48-55 | tax 56-63
 *   w4 (u32): shipdate - sd_base bits 0-15 | group code 16-18 (0..5 =
 *             fi*2+si as k_q1_agg computes it, 7 = unexpected flag byte)
 */
#ifndef GG_Q1_PACK_H
#define GG_Q1_PACK_H

#include <cstdint>

namespace gg
{

static constexpr int Q1P_THREADS = 256;		/* block of the packed scan */
static constexpr int Q1P_ROWS = 4;		/* rows per lane and load */
static constexpr int64_t Q1P_MAX_BLOCKS = 2048;	/* default grid ceiling */
static constexpr uint32_t Q1P_BAD_CODE = 7;

/* signed min/max of the five narrowed columns (engine_col_minmax) */
struct Q1PackRanges
{
	long long qmin, qmax;	/* qty */
	long long pmin, pmax;	/* price */
	long long dmin, dmax;	/* disc */
	long long tmin, tmax;	/* tax */
	long long sdmin, sdmax;	/* shipdate */
};

/* every value fits its field, and 100 - disc cannot go negative */
static inline bool q1_pack_eligible(int64_t nrows, const Q1PackRanges &r)
{
	if (nrows <= 0)
		return false;
	if (r.qmin < 0 || r.qmax > 65535)
		return false;
	if (r.pmin < 0 || r.pmax > 4294967295ll)
		return false;
	if (r.dmin < 0 || r.dmax > 100)
		return false;
	if (r.tmin < 0 || r.tmax > 255)
		return false;
	/* both ends are int32 values: the span fits 64 bits */
	if (r.sdmax - r.sdmin > 65535)
		return false;
	return true;
}

/* the most one row adds to the widest sum, charge6 = p*(100-d)*(100+t):
 * at most (2^32-1) * 100 * 355 < 2^48 for an eligible table */
static inline uint64_t q1_pack_row_bound(long long pmax, long long tmax)
{
	return (uint64_t) pmax * 100u * (uint64_t) (100 + tmax);
}

/* quads (4-row groups, the last one possibly short) of an n-row table */
static inline int64_t q1_pack_quads(int64_t n)
{
	return (n + Q1P_ROWS - 1) / Q1P_ROWS;
}

/* rows one block of a `grid`-block packed scan accumulates, at most: its
 * grid-stride iterations over whole quads, plus the short tail (< 4 rows)
 * that one thread of block 0 adds */
static inline int64_t q1_pack_rows_per_block(int64_t n, int64_t grid)
{
	int64_t per_iter = grid * Q1P_THREADS;
	int64_t iters = (q1_pack_quads(n) + per_iter - 1) / per_iter;

	return iters * Q1P_THREADS * Q1P_ROWS + (Q1P_ROWS - 1);
}

/* does rows_per_block * row_bound stay below 2^64 at this grid? */
static inline bool q1_pack_grid_ok(int64_t n, int64_t grid,
				   uint64_t row_bound)
{
	unsigned __int128 tot = (unsigned __int128)
		(uint64_t) q1_pack_rows_per_block(n, grid) * row_bound;

	return (tot >> 64) == 0;
}

/* Blocks for the packed scan of n > 0 rows.  want <= 0 asks for the
 * default (one quad per lane, at most Q1P_MAX_BLOCKS); a forced grid is
 * clamped to [floor, cap], where cap gives every lane at most one quad and
 * floor is the smallest grid whose per-block u64 partials cannot wrap.
 * floor <= cap for every eligible table: one iteration is 1027 rows at
 * most, and 1027 * 2^48 < 2^64. */
static inline int64_t q1_pack_grid(int64_t n, int64_t want,
				   uint64_t row_bound)
{
	int64_t quads = q1_pack_quads(n);
	int64_t cap = (quads + Q1P_THREADS - 1) / Q1P_THREADS;
	int64_t g, floor_g = 1;

	if (cap < 1)
		cap = 1;
	if (row_bound)
	{
		/* rows a block may take, then whole iterations of it */
		uint64_t rows = ~0ull / row_bound;
		uint64_t iters = rows < (uint64_t) (Q1P_ROWS - 1) ? 0
			: (rows - (Q1P_ROWS - 1)) / (Q1P_THREADS * Q1P_ROWS);

		if (iters < 1)
			iters = 1;	/* not reached when eligible */
		if (iters > (1ull << 40))
			iters = 1ull << 40;
		floor_g = (int64_t) (((uint64_t) quads +
				      iters * Q1P_THREADS - 1) /
				     (iters * Q1P_THREADS));
		if (floor_g < 1)
			floor_g = 1;
	}
	g = want > 0 ? want : (cap < Q1P_MAX_BLOCKS ? cap : Q1P_MAX_BLOCKS);
	if (g < floor_g)
		g = floor_g;
	if (g > cap)
		g = cap;
	return g;
}

/* The cutoff in the kernel's domain, c = cutoff - sd_base: false when no
 * row can pass (c < 0); otherwise *c is clamped to 65535, which every
 * stored date offset satisfies. */
static inline bool q1_pack_cutoff(int32_t cutoff, int32_t sd_base,
				  uint32_t *c)
{
	int64_t d = (int64_t) cutoff - (int64_t) sd_base;

	if (d < 0)
		return false;
	*c = d > 65535 ? 65535u : (uint32_t) d;
	return true;
}

}				/* namespace gg */

#endif
