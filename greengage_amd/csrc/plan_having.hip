/*
 * Device HAVING over a compiled plan's compacted group rows (engine_abi.h
 * gg_plan_having): the qual of the Agg node (nodeAgg.c: ExecQual over the
 * projected aggregates), evaluated where the groups already are, between
 * the compaction and the device top-k.
 *
 * k_plan_having_select walks the ng rows (code, naggs x (lo, hi)) with the
 * plan kernels' grid (pl_grid), tests each with plan_having_row
 * (plan_having.h, the host path's own test) and appends the indices of the
 * rows that pass to a uint32 list.  The atoms live in the kernel arguments,
 * so their kinds and slots are wave-uniform and a row reads only the words
 * the atoms name.  The append is aggregated: a ballot and popcount per wave,
 * the wave counts combined through LDS, and ONE atomicAdd on the global
 * counter per block and stride step, skipped when no row of the block
 * passed.  Under a selective HAVING almost every step issues none.  The
 * list's order is unspecified; the plan's total order decides the result.
 *
 * k_plan_having_gather copies the listed rows out, for the plans whose
 * survivors all go to the host (the top-k's own gather stops at its limit).
 */
#include <hip/hip_runtime.h>

#include "engine_internal.h"

namespace gg
{

static constexpr int PL_HV_THREADS = 256;
static constexpr int PL_HV_WAVES = PL_HV_THREADS / 64;	/* wave64 */

__global__ __launch_bounds__(PL_HV_THREADS)
void k_plan_having_select(PlanHavingDev H,
			  const unsigned long long *__restrict__ rows,
			  uint64_t ng, int rowsz, uint32_t *__restrict__ idx,
			  unsigned long long *ctr)
{
	/* two sets, used by alternate steps: a step's reads of its set end
	 * before any thread passes the next step's first barrier, and that
	 * set is next written only after it */
	__shared__ unsigned int wcnt[2][PL_HV_WAVES];
	__shared__ unsigned long long bbase[2];
	const uint64_t stride = (uint64_t) gridDim.x * PL_HV_THREADS;
	const int lane = (int) (threadIdx.x & 63);
	const int wave = (int) (threadIdx.x >> 6);
	int par = 0;

	/* the bound is block-uniform: every thread of a block takes the same
	 * steps, so the barriers inside are safe */
	for (uint64_t b = (uint64_t) blockIdx.x * PL_HV_THREADS; b < ng;
	     b += stride, par ^= 1)
	{
		const uint64_t i = b + threadIdx.x;
		const bool pass = i < ng &&
			plan_having_row(H, rows + i * (uint64_t) rowsz);
		const unsigned long long mask = __ballot(pass);

		if (lane == 0)
			wcnt[par][wave] = (unsigned int) __popcll(mask);
		__syncthreads();
		if (threadIdx.x == 0)
		{
			unsigned int tot = 0;

			for (int w = 0; w < PL_HV_WAVES; w++)
				tot += wcnt[par][w];
			if (tot)
				bbase[par] = atomicAdd(ctr,
						       (unsigned long long) tot);
		}
		__syncthreads();
		if (pass)
		{
			unsigned long long at = bbase[par] +
				(unsigned long long) __popcll(
					mask & ((1ull << lane) - 1));

			for (int w = 0; w < wave; w++)
				at += wcnt[par][w];
			if (at < ng)	/* always: at most ng rows pass */
				idx[at] = (uint32_t) i;
		}
	}
}

hipError_t launch_plan_having_select(hipStream_t s, const PlanHavingDev &H,
				     const unsigned long long *rows,
				     uint64_t ng, int rowsz, uint32_t *idx,
				     unsigned long long *ctr)
{
	if (ng >= PL_TOPK_PAD || rowsz < 1 || H.nclauses < 1 ||
	    H.nclauses > GG_PLAN_MAX_HAVING_CLAUSES)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_plan_having_select, dim3(pl_grid((int64_t) ng)),
			   dim3(PL_HV_THREADS), 0, s, H, rows, ng, rowsz, idx,
			   ctr);
	return hipGetLastError();
}

__global__ __launch_bounds__(PL_HV_THREADS)
void k_plan_having_gather(const unsigned long long *__restrict__ rows,
			  uint64_t ng, int rowsz,
			  const uint32_t *__restrict__ idx, uint64_t ns,
			  unsigned long long *__restrict__ out)
{
	const uint64_t total = ns * (uint64_t) rowsz;
	const uint64_t stride = (uint64_t) gridDim.x * PL_HV_THREADS;

	for (uint64_t t = (uint64_t) blockIdx.x * PL_HV_THREADS + threadIdx.x;
	     t < total; t += stride)
	{
		const uint64_t r = idx[t / rowsz];

		out[t] = r < ng ? rows[r * (uint64_t) rowsz + t % rowsz] : 0;
	}
}

hipError_t launch_plan_having_gather(hipStream_t s,
				     const unsigned long long *rows,
				     uint64_t ng, int rowsz,
				     const uint32_t *idx, uint64_t ns,
				     unsigned long long *out)
{
	if (ns > ng || rowsz < 1)
		return hipErrorInvalidValue;
	if (ns == 0)
		return hipSuccess;
	hipLaunchKernelGGL(k_plan_having_gather,
			   dim3(pl_grid((int64_t) (ns * (uint64_t) rowsz))),
			   dim3(PL_HV_THREADS), 0, s, rows, ng, rowsz, idx, ns,
			   out);
	return hipGetLastError();
}

}				/* namespace gg */
