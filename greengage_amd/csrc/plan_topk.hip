/*
 * Device top-k over a compiled plan's compacted group rows
 * (engine_abi.h gg_plan_order / gg_plan_desc.limit): the first `limit`
 * rows under the plan's order, selected by a tournament of bitonic sorts.
 *
 * A round cuts its candidates into tiles of PL_TOPK_TILE row indices, one
 * workgroup per tile.  The tile extracts each candidate's SORT KEY into LDS
 * once, bitonic-sorts a permutation of its slots by those keys and writes
 * the row indices of its first `limit` slots.  The survivors are the next
 * round's candidates, until one tile is left, whose head is the answer.  A
 * tile holds at least 2 * limit candidates, so every round at least halves
 * them; only the first round reads all the rows, and of each row only the
 * words the order names.
 *
 * Sort key = 2 * norder + 1 u64 words, compared as unsigned, most
 * significant first, smaller = earlier in the result:
 *   per order entry, two words
 *     group key / MIN / MAX   (is_null XOR nulls_first, value), value =
 *                             the int64 with its sign bit flipped,
 *                             complemented for DESC, 0 for a NULL
 *     COUNT / SUM             (hi with its sign bit flipped, lo) of the
 *                             signed 128-bit value, both complemented for
 *                             DESC
 *   then one tie-break word that orders as (key0, key1) ascending does
 *   (pl_tie_word).
 * This encodes, entry for entry, the comparator plan.cpp defines
 * (plan_order_cmp); plan.cpp runs the rows that come back through that
 * comparator once more, which keeps it the single definition of the order.
 * Rows are distinct groups, so no two keys of real rows are equal and the
 * result does not depend on how a tile's rows were laid out.
 *
 * LDS: keys are stored word-major (word w of slot s at w * TILE + s), so
 * the extraction's stores and a compare's first loads fall on consecutive
 * banks for consecutive slots; the permutation is TILE uint16 (slot, bit 15
 * = padding).  Bytes per tile = TILE * (8 * (2 * norder + 1) + 2): 53,248
 * for one entry, 151,552 for four, against 160 KiB per CU.  DESIGN.md
 * "ORDER BY / LIMIT" has the occupancy reasoning.
 */
#include <hip/hip_runtime.h>

#include "engine_internal.h"

namespace gg
{

extern "C" int
gg_engine_plan_topk_tile(void)
{
	return PL_TOPK_TILE;
}

size_t plan_topk_lds_bytes(int norder)
{
	return (size_t) PL_TOPK_TILE * (8 * (2 * (size_t) norder + 1) + 2);
}

/* one word that orders the rows as (key0, key1, ...) ascending does, NULL keys
 * (GG_PLAN_NULL_KEY, the smallest int64 a key can be) first */
__device__ static inline unsigned long long
pl_tie_word(const PlanTopkDev &K, unsigned long long code)
{
	if (K.gp.packed || K.kn.n >= 3)
		/* e = 0 for NULL, else the offset from the column minimum
		 * plus 1: the packed code, of two fields or of N with field 0
		 * most significant, is already monotone in all its keys */
		return code;
	if (K.ngroup == 2)
	{
		/* char1 pair: NULL is 256 in the code, first in the order */
		unsigned long long e0 = code / 512, e1 = code % 512;

		return (e0 == 256 ? 0 : e0 + 1) * 512 + (e1 == 256 ? 0 : e1 + 1);
	}
	return code ^ PL_MSB;	/* the key itself, signed */
}

/* the two key words of order entry E for one compacted row */
__device__ static inline void
pl_order_words(const PlanTopkDev &K, const PlanOrderEnt &E,
	       const unsigned long long *row, unsigned long long *w0,
	       unsigned long long *w1)
{
	const unsigned long long flip = E.desc ? ~0ull : 0ull;

	if (E.kind == PL_ORD_I128)
	{
		*w0 = (row[2 + 2 * E.slot] ^ PL_MSB) ^ flip;
		*w1 = row[1 + 2 * E.slot] ^ flip;
		return;
	}
	bool null;
	unsigned long long v;

	if (E.kind == PL_ORD_KEY)
	{
		int64_t k[PL_MAX_GCOLS];

		plan_keys_of(K.gp, K.kn, K.ngroup, (long long) row[0], k);
		null = k[E.slot] == GG_PLAN_NULL_KEY;
		v = (unsigned long long) k[E.slot] ^ PL_MSB;
	}
	else
	{
		/* the MAX word is x ^ MSB, the MIN word its complement
		 * (plan_dev.h PlanAggDev): x ^ MSB is the word wanted */
		unsigned long long e = row[1 + 2 * E.slot];

		null = row[1 + 2 * E.cnt] == 0;
		v = E.kind == PL_ORD_MIN ? ~e : e;
	}
	*w0 = (unsigned long long) (null != (E.nulls_first != 0));
	*w1 = null ? 0 : v ^ flip;
}

/* slot a before slot b?  Padding (bit 15) goes last. */
__device__ static inline bool
pl_topk_less(const unsigned long long *keys, int kw, unsigned a, unsigned b)
{
	if ((a | b) & 0x8000u)
		return (a & 0x8000u) < (b & 0x8000u);
	for (int w = 0; w < kw; w++)
	{
		unsigned long long x = keys[w * PL_TOPK_TILE + a];
		unsigned long long y = keys[w * PL_TOPK_TILE + b];

		if (x != y)
			return x < y;
	}
	return false;
}

__global__ __launch_bounds__(PL_TOPK_THREADS)
void k_plan_topk_round(PlanTopkDev K, const uint32_t *__restrict__ src,
		       uint64_t n, uint32_t *__restrict__ dst)
{
	extern __shared__ unsigned long long pl_topk_lds[];
	const int kw = 2 * K.norder + 1;
	unsigned long long *keys = pl_topk_lds;
	unsigned short *perm = (unsigned short *) (keys + (size_t) kw *
						   PL_TOPK_TILE);
	const uint64_t base = (uint64_t) blockIdx.x * PL_TOPK_TILE;

	/* 1. sort keys of this tile's candidates */
	for (unsigned s = threadIdx.x; s < PL_TOPK_TILE; s += blockDim.x)
	{
		uint64_t pos = base + s;
		uint64_t r = PL_TOPK_PAD;

		if (pos < n)
			r = src ? src[pos] : pos;
		if (r >= K.ng)		/* padding (or nothing to read) */
		{
			perm[s] = (unsigned short) (s | 0x8000u);
			continue;
		}
		const unsigned long long *row = K.rows + r * (uint64_t) K.rowsz;

		for (int o = 0; o < K.norder; o++)
		{
			unsigned long long w0, w1;

			pl_order_words(K, K.ord[o], row, &w0, &w1);
			keys[(2 * o) * PL_TOPK_TILE + s] = w0;
			keys[(2 * o + 1) * PL_TOPK_TILE + s] = w1;
		}
		keys[(kw - 1) * PL_TOPK_TILE + s] = pl_tie_word(K, row[0]);
		perm[s] = (unsigned short) s;
	}
	__syncthreads();

	/* 2. bitonic sort of the permutation, ascending */
	for (unsigned k = 2; k <= PL_TOPK_TILE; k <<= 1)
		for (unsigned j = k >> 1; j > 0; j >>= 1)
		{
			for (unsigned t = threadIdx.x; t < PL_TOPK_TILE / 2;
			     t += blockDim.x)
			{
				unsigned i = 2 * t - (t & (j - 1));
				unsigned l = i + j;
				unsigned a = perm[i], b = perm[l];
				bool up = (i & k) == 0;

				if (up ? pl_topk_less(keys, kw, b & 0x87FFu,
						      a & 0x87FFu)
				    : pl_topk_less(keys, kw, a & 0x87FFu,
						   b & 0x87FFu))
				{
					perm[i] = (unsigned short) b;
					perm[l] = (unsigned short) a;
				}
			}
			__syncthreads();
		}

	/* 3. the head of the tile, as row indices */
	for (unsigned j = threadIdx.x; j < (unsigned) K.limit; j += blockDim.x)
	{
		unsigned p = perm[j];
		uint32_t r = PL_TOPK_PAD;

		if (!(p & 0x8000u))
		{
			uint64_t pos = base + (p & 0x7FFu);

			r = src ? src[pos] : (uint32_t) pos;
		}
		dst[(uint64_t) blockIdx.x * K.limit + j] = r;
	}
}

hipError_t launch_plan_topk_round(hipStream_t s, const PlanTopkDev &K,
				  const uint32_t *src, uint64_t n,
				  uint32_t *dst)
{
	const size_t lds = plan_topk_lds_bytes(K.norder);
	const uint64_t tiles = (n + PL_TOPK_TILE - 1) / PL_TOPK_TILE;
	hipError_t rc;

	if (K.norder < 0 || K.norder > GG_PLAN_MAX_ORDER || K.limit < 1 ||
	    K.limit > GG_PLAN_MAX_LIMIT || tiles < 1 || tiles > 0x7FFFFFFFull ||
	    K.ng >= PL_TOPK_PAD)
		return hipErrorInvalidValue;
	rc = hipFuncSetAttribute((const void *) k_plan_topk_round,
				 hipFuncAttributeMaxDynamicSharedMemorySize,
				 (int) lds);
	if (rc != hipSuccess)
		return rc;
	hipLaunchKernelGGL(k_plan_topk_round, dim3((unsigned) tiles),
			   dim3(PL_TOPK_THREADS), lds, s, K, src, n, dst);
	return hipGetLastError();
}

__global__ __launch_bounds__(256)
void k_plan_topk_gather(PlanTopkDev K, const uint32_t *__restrict__ idx,
			unsigned long long *__restrict__ out)
{
	const int total = K.limit * K.rowsz;

	for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total;
	     t += gridDim.x * blockDim.x)
	{
		uint64_t r = idx[t / K.rowsz];

		out[t] = r < K.ng
			? K.rows[r * (uint64_t) K.rowsz + t % K.rowsz] : 0;
	}
}

hipError_t launch_plan_topk_gather(hipStream_t s, const PlanTopkDev &K,
				   const uint32_t *idx,
				   unsigned long long *out)
{
	const int total = K.limit * K.rowsz;

	hipLaunchKernelGGL(k_plan_topk_gather, dim3((total + 255) / 256),
			   dim3(256), 0, s, K, idx, out);
	return hipGetLastError();
}

}				/* namespace gg */
