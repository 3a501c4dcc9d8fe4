/*
 * Device regroup behind a compiled plan with a COUNT(DISTINCT) aggregate
 * (engine_abi.h gg_plan_aggkind; plan_distinct.h holds the fold's two
 * functions, which the host path shares): the outer Agg of the reference's
 * two-stage plan (cdbgroup.c), a second group-by over the inner plan's
 * compacted groups, one per (group key, value) pair, by the group key alone.
 * It runs between the compaction and the device HAVING / top-k, so only the
 * rows the plan emits are copied back.
 *
 * k_plan_regroup walks the ng_in rows (code, naggs x (lo, hi)) on the plan
 * kernels' grid (pl_grid).  A thread decodes its row's outer code
 * (plan_regroup_code) and folds the row's contributions
 * (plan_regroup_contrib) through a per-block LDS group cache built like the
 * one of k_plan_scan_agg: 32 slots, open addressing by gg_hashint8, at most
 * 8 probes, 8 replicas chosen by threadIdx.x & 7.  The shape that matters is
 * "distinct customers per nation": millions of pairs into 25 groups, where
 * per-row global atomics on a handful of accumulator words would sit on the
 * hot-word wall that cache exists to avoid.  A row whose code finds no cache
 * slot goes straight to the global table (pl_slot), and the cache is flushed
 * once per occupied slot at block end: the replicas folded, zeros skipped,
 * one atomic per slot word.  Every row finds or creates its outer group,
 * whatever it contributes: a group whose values are all NULL exists, with
 * count 0.
 *
 * The slot kinds and the distinct mask live in the kernel arguments, so they
 * are wave-uniform.  launch_plan_compact over the outer table finishes the
 * fold: outer rows of the same row size.
 */
#include <hip/hip_runtime.h>

#include "../../include/gg_pg_hash.h"
#include "engine_internal.h"

namespace gg
{

static constexpr int PL_RG_THREADS = 256;	/* pl_grid's block */
static constexpr int PL_RG_SLOTS = 32;
static constexpr int PL_RG_REPL = 8;

/* one contribution into the accumulator w[0..1], in LDS or global memory */
__device__ static inline void
pl_regroup_apply(int kind, unsigned long long *w, unsigned long long vlo,
		 unsigned long long vhi)
{
	if (kind >= 3)
		atomicMax(w, vlo);
	else
		pl_atomic_add128(w, vlo, vhi);
}

__global__ __launch_bounds__(PL_RG_THREADS)
void k_plan_regroup(PlanRegroupDev G,
		    const unsigned long long *__restrict__ rows, uint64_t ng_in,
		    int rowsz, unsigned long long *tkeys,
		    unsigned long long *tvals, uint64_t nslots,
		    unsigned long long *err)
{
	constexpr long long LEMPTY = (long long) PL_EMPTY;
	__shared__ long long lkeys[PL_RG_SLOTS];
	__shared__ unsigned long long
		lvals[PL_RG_REPL][PL_RG_SLOTS][2 * GG_PLAN_MAX_AGGS];
	const uint64_t stride = (uint64_t) gridDim.x * PL_RG_THREADS;
	const int lrep = (int) (threadIdx.x & (PL_RG_REPL - 1));
	/* pl_slot reads the table's two fields of a PlanDev and no other */
	PlanDev T;

	T.tkeys = tkeys;
	T.nslots = nslots;

	for (int s = threadIdx.x; s < PL_RG_SLOTS; s += PL_RG_THREADS)
		lkeys[s] = LEMPTY;
	for (int s = threadIdx.x;
	     s < PL_RG_REPL * PL_RG_SLOTS * 2 * GG_PLAN_MAX_AGGS;
	     s += PL_RG_THREADS)
		((unsigned long long *) lvals)[s] = 0;
	__syncthreads();

	for (uint64_t i = (uint64_t) blockIdx.x * PL_RG_THREADS + threadIdx.x;
	     i < ng_in; i += stride)
	{
		const unsigned long long *row = rows + i * (uint64_t) rowsz;
		const long long code = plan_regroup_code(G, (long long) row[0]);
		int ls = -1;
		uint32_t pos = (uint32_t) gg_hashint8(code) & (PL_RG_SLOTS - 1);

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
				long long prev = (long long) atomicCAS(
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
			pos = (pos + 1) & (PL_RG_SLOTS - 1);
		}
		/* called once per address space, so each call's atomics are
		 * LDS or global ones, not flat */
		auto fold = [&](unsigned long long *acc)
		{
			for (int a = 0; a < G.naggs; a++)
			{
				unsigned long long vlo, vhi;

				if (plan_regroup_contrib(G, a, row[1 + 2 * a],
							 row[2 + 2 * a], &vlo,
							 &vhi))
					pl_regroup_apply(G.kind[a], &acc[2 * a],
							 vlo, vhi);
			}
		};

		if (ls >= 0)
		{
			fold(lvals[lrep][ls]);
			continue;
		}
		/* cache full: straight into the global table */
		int64_t slot = pl_slot(T, code);

		if (slot < 0)
		{
			atomicOr(err, PL_ERR_FULL);
			continue;
		}
		fold(&tvals[(uint64_t) slot * G.naggs * 2]);
	}

	/* flush the block's LDS groups into the global table */
	__syncthreads();
	for (int s = threadIdx.x; s < PL_RG_SLOTS; s += PL_RG_THREADS)
	{
		if (lkeys[s] == LEMPTY)
			continue;
		int64_t slot = pl_slot(T, lkeys[s]);

		if (slot < 0)
		{
			atomicOr(err, PL_ERR_FULL);
			continue;
		}
		for (int a = 0; a < G.naggs; a++)
		{
			unsigned long long *dst =
				&tvals[((uint64_t) slot * G.naggs + a) * 2];
			unsigned long long lo = 0, hi = 0;

			if (G.kind[a] >= 3)
			{
				for (int rr = 0; rr < PL_RG_REPL; rr++)
					if (lvals[rr][s][2 * a] > lo)
						lo = lvals[rr][s][2 * a];
				if (lo)
					atomicMax(dst, lo);
				continue;
			}
			for (int rr = 0; rr < PL_RG_REPL; rr++)
				pl_add128(lo, hi, lvals[rr][s][2 * a],
					  lvals[rr][s][2 * a + 1]);
			if (lo || hi)
				pl_atomic_add128(dst, lo, hi);
		}
	}
	/* a plan without a group column: its one group exists, rows or not
	 * (every code is 0 and nslots is 1) */
	if (G.ngroup < 2 && blockIdx.x == 0 && threadIdx.x == 0)
		tkeys[0] = 0;
}

hipError_t launch_plan_regroup(hipStream_t s, const PlanRegroupDev &G,
			       const unsigned long long *rows, uint64_t ng_in,
			       int rowsz, unsigned long long *tkeys,
			       unsigned long long *tvals, uint64_t nslots,
			       unsigned long long *err)
{
	if (G.naggs < 1 || G.naggs > GG_PLAN_MAX_AGGS ||
	    rowsz != 1 + 2 * G.naggs || G.ngroup < 1 || G.ngroup > 2 ||
	    nslots == 0 || (nslots & (nslots - 1)) != 0)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_plan_regroup, dim3(pl_grid((int64_t) ng_in)),
			   dim3(PL_RG_THREADS), 0, s, G, rows, ng_in, rowsz,
			   tkeys, tvals, nslots, err);
	return hipGetLastError();
}

}				/* namespace gg */
