/*
 * Host-side arithmetic of the packed Q1 companion ("Packed Q1
 * companion"): which tables may be narrowed, how many blocks the packed
 * scan needs so that a block's u64 partial sums cannot wrap, and the
 * cutoff in the 16-bit shipdate domain.  Plain functions with no HIP
 * dependency: engine_abi.cpp and kernels.hip use them, and
 * tests/test_q1_pack_cpu.py and tests/test_q1_pack8_cpu.py compile them
 * into stand-alone programs.
 *
 * Layout, one entry per row:
 *   w8 (u64): price bits 0-31 | qty 32-47 | disc 48-55 | tax 56-63
 *   w4 (u32): shipdate - sd_base bits 0-15 | group code 16-18 (0..5 =
 *             fi*2+si as k_q1_agg computes it, 7 = unexpected flag byte)
 *
 * The 8 B tier (second half of this file) holds a row in w8 alone when the
 * bit lengths of the table's own maxima fit: from bit 0 upwards
 *   shipdate - sd_base | code (3 bits) | disc | tax | qty | price
 * each field bits(max) wide, bits(0) = 0 (Q1Pack8Layout).  At TPC-H ranges
 * that is 12 + 3 + 4 + 4 + 13 + 24 = 60 bits.
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

/* ------------------------------------------------------------------ */
/* The 8 B tier: one u64 per row when the table's own ranges fit       */
/* ------------------------------------------------------------------ */

#ifdef __HIPCC__
#define GG_Q1P_HD __host__ __device__
#else
#define GG_Q1P_HD
#endif

static constexpr int64_t Q1P8_MIN_ROWS = 1024;	/* below it, stay at 12 B */

/* Shifts and masks of the u64, computed once per table from its ranges
 * and passed to both kernels by value.  No shift reaches 64 (the fields
 * below price are at most 16 + 3 + 7 + 8 + 16 = 50 bits); a zero-width
 * field has mask 0.  The shipdate offset sits at bit 0. */
struct Q1Pack8Layout
{
	uint32_t sd_mask;
	uint32_t code_shift;		/* 3 bits, inside the low dword */
	uint32_t d_shift, d_mask;	/* inside the low dword */
	uint32_t t_shift, t_mask;
	uint32_t q_shift, q_mask;
	uint32_t p_shift, p_mask;	/* on top: a bare shift unpacks it */
	uint32_t bits;			/* all six widths, <= 64 */
};

/* bit length; 0 for 0 */
static inline int q1_pack8_bits(unsigned long long x)
{
	int b = 0;

	for (; x; x >>= 1)
		b++;
	return b;
}

/* widths of an eligible (q1_pack_eligible) table's six fields, summed */
static inline int q1_pack8_width(const Q1PackRanges &r)
{
	return q1_pack8_bits((unsigned long long) r.qmax) +
		q1_pack8_bits((unsigned long long) r.pmax) +
		q1_pack8_bits((unsigned long long) r.dmax) +
		q1_pack8_bits((unsigned long long) r.tmax) +
		q1_pack8_bits((unsigned long long) (r.sdmax - r.sdmin)) + 3;
}

/* a subset of the 12 B tier: the widths fit one u64, and the table is at
 * least one block-iteration long */
static inline bool q1_pack8_eligible(int64_t nrows, const Q1PackRanges &r)
{
	if (!q1_pack_eligible(nrows, r) || nrows < Q1P8_MIN_ROWS)
		return false;
	return q1_pack8_width(r) <= 64;
}

static inline uint32_t q1_pack8_mask(int bits)
{
	return bits >= 32 ? 0xFFFFFFFFu : (1u << bits) - 1u;
}

/* the layout of a q1_pack8_eligible table */
static inline Q1Pack8Layout q1_pack8_layout(const Q1PackRanges &r)
{
	const int sb = q1_pack8_bits((unsigned long long) (r.sdmax - r.sdmin));
	const int db = q1_pack8_bits((unsigned long long) r.dmax);
	const int tb = q1_pack8_bits((unsigned long long) r.tmax);
	const int qb = q1_pack8_bits((unsigned long long) r.qmax);
	const int pb = q1_pack8_bits((unsigned long long) r.pmax);
	Q1Pack8Layout l;

	l.sd_mask = q1_pack8_mask(sb);
	l.code_shift = (uint32_t) sb;
	l.d_shift = l.code_shift + 3;
	l.d_mask = q1_pack8_mask(db);
	l.t_shift = l.d_shift + (uint32_t) db;
	l.t_mask = q1_pack8_mask(tb);
	l.q_shift = l.t_shift + (uint32_t) tb;
	l.q_mask = q1_pack8_mask(qb);
	l.p_shift = l.q_shift + (uint32_t) qb;
	l.p_mask = q1_pack8_mask(pb);
	l.bits = l.p_shift + (uint32_t) pb;
	return l;
}

/* one row's word; every value is inside its field (the host proved it) */
GG_Q1P_HD static inline unsigned long long
q1_pack8_word(const Q1Pack8Layout &l, uint32_t sd_off, uint32_t code,
	      uint32_t d, uint32_t t, uint32_t q, uint32_t p)
{
	return (unsigned long long) (sd_off & l.sd_mask) |
		((unsigned long long) (code & 7u) << l.code_shift) |
		((unsigned long long) (d & l.d_mask) << l.d_shift) |
		((unsigned long long) (t & l.t_mask) << l.t_shift) |
		((unsigned long long) (q & l.q_mask) << l.q_shift) |
		((unsigned long long) (p & l.p_mask) << l.p_shift);
}

/* the fields of a word; price needs no mask, nothing lies above it */
GG_Q1P_HD static inline uint32_t
q1_pack8_sd(const Q1Pack8Layout &l, unsigned long long w)
{
	return (uint32_t) w & l.sd_mask;
}
GG_Q1P_HD static inline uint32_t
q1_pack8_code(const Q1Pack8Layout &l, unsigned long long w)
{
	return ((uint32_t) w >> l.code_shift) & 7u;
}
GG_Q1P_HD static inline uint32_t
q1_pack8_disc(const Q1Pack8Layout &l, unsigned long long w)
{
	return ((uint32_t) w >> l.d_shift) & l.d_mask;
}
GG_Q1P_HD static inline uint32_t
q1_pack8_tax(const Q1Pack8Layout &l, unsigned long long w)
{
#ifdef __HIP_DEVICE_COMPILE__
	/* t_shift <= 26: one funnel shift instead of a 64-bit one */
	return __builtin_amdgcn_alignbit((uint32_t) (w >> 32), (uint32_t) w,
					 l.t_shift) & l.t_mask;
#else
	return (uint32_t) (w >> l.t_shift) & l.t_mask;
#endif
}
GG_Q1P_HD static inline uint32_t
q1_pack8_qty(const Q1Pack8Layout &l, unsigned long long w)
{
	return (uint32_t) (w >> l.q_shift) & l.q_mask;
}
GG_Q1P_HD static inline uint32_t
q1_pack8_price(const Q1Pack8Layout &l, unsigned long long w)
{
	return (uint32_t) (w >> l.p_shift);
}

/* q1_pack_cutoff in the 8 B tier's shipdate field: clamped to the field's
 * own maximum, which every stored offset satisfies */
static inline bool q1_pack8_cutoff(int32_t cutoff, int32_t sd_base,
				   uint32_t sd_mask, uint32_t *c)
{
	int64_t d = (int64_t) cutoff - (int64_t) sd_base;

	if (d < 0)
		return false;
	*c = d > (int64_t) sd_mask ? sd_mask : (uint32_t) d;
	return true;
}

/*
 * Folding count, sum(disc) and sum(qty) of one LDS replica into one u64
 * word (four LDS adds per row instead of six): sum(qty) in the high dword,
 * sum(disc) in the low dword from d_shift up, the count below it.  A
 * replica is fed by the 8 lanes of a block with lane % 32 == r, each at
 * most `iters` quads, plus the short tail in replica 0; the sums of that
 * many rows must fit their parts.  `on` = 0 keeps six adds.
 */
struct Q1Pack8Fold
{
	uint32_t on;
	uint32_t d_shift;	/* 1..31 when on */
};

static inline int64_t q1_pack8_rows_per_replica(int64_t n, int64_t grid)
{
	return (q1_pack_rows_per_block(n, grid) - (Q1P_ROWS - 1)) / 32 +
		(Q1P_ROWS - 1);
}

static inline Q1Pack8Fold q1_pack8_fold(int64_t n, int64_t grid,
					long long qmax, long long dmax)
{
	Q1Pack8Fold f = {0, 0};
	const int64_t rows = q1_pack8_rows_per_replica(n, grid);

	if (rows < 1 || rows > 0x7FFFFFFFll || qmax < 0 || qmax > 65535 ||
	    dmax < 0 || dmax > 100)
		return f;
	const int cb = q1_pack8_bits((unsigned long long) rows);
	const int db = q1_pack8_bits((unsigned long long) rows *
				     (unsigned long long) dmax);
	const int qb = q1_pack8_bits((unsigned long long) rows *
				     (unsigned long long) qmax);

	if (cb + db > 32 || qb > 32)
		return f;
	f.on = 1;
	f.d_shift = (uint32_t) cb;	/* rows >= 1: 1 <= cb <= 31 */
	return f;
}

}				/* namespace gg */

#endif
