/*
 * MI355X (gfx950, CDNA4) kernels for the hot path — written for 64-wide
 * wavefronts, LDS-privatized accumulators, coalesced 8-byte column
 * streams from HBM.  No MFMA: every kernel here is HBM-bandwidth-bound
 * gather/scan work (SURVEY §8(d) roofline).
 *
 * Reference semantics implemented (cited per kernel):
 *   k_q1_agg          execScan.c:110–214 + execHHashagg.c:905–1081 +
 *                     nodeAgg.c:393–860 (scan+filter+group agg, exact
 *                     scaled-int arithmetic)
 *   k_q1_agg_packed   the same query over the 12 B/row companion that
 *                     k_q1_pack_build writes once per table (q1_pack.h)
 *   k_q1_agg_packed8  the same over the companion's 8 B/row tier, written
 *                     by k_q1_pack8_build when the table's ranges fit a u64
 *   k_build_* / k_probe_*  nodeHash.c:88–176/:905/:1002, nodeHashjoin.c:
 *                     78–510 (hash build/probe; open addressing instead
 *                     of chained buckets — GPU-native layout, same join
 *                     row-set semantics; rows a5–a7)
 *   k_sumprice        BASELINE config 1
 *   k_gen_*           include/gg_gen.h (deterministic synthetic data)
 *   k_part_*          nodeMotion.c:1574 doSendTuple hash routing via
 *                     bit-exact cdbhash (include/gg_pg_hash.h; row a11)
 */
#include <hip/hip_runtime.h>
#include <cstdlib>

#include "../../include/gg_pg_hash.h"
#include "../../include/gg_gen.h"
#include "../../include/gg_checksum.h"
#include "engine_internal.h"
#include "q1_pack.h"

namespace gg
{

static constexpr int THREADS = 256;
/* 256 CUs × 8 blocks of 256 threads per CU (Guideline 11) */
static constexpr int MAX_BLOCKS = 2048;

/* nontemporal loads for read-once streams (bypass L1, early L2 evict;
 * never used on hash-table / bloom traffic, which wants caching) */
__device__ inline int64_t nt_ld64(const int64_t *p)
{
	return __builtin_nontemporal_load(p);
}
__device__ inline int32_t nt_ld32(const int32_t *p)
{
	return __builtin_nontemporal_load(p);
}

static inline int grid_for(int64_t n)
{
	int64_t b = (n + THREADS - 1) / THREADS;

	return (int) (b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

/* ------------------------------------------------------------------ */
/* Q1: fused scan + predicate + 6-group aggregation                    */
/* ------------------------------------------------------------------ */

/* LDS accumulator: 32 replicas (lane % 32) × 6 groups × 8 fields,
 * replica stride padded to 49 u64 so consecutive replicas land on
 * different LDS banks for the b64 atomics. */
static constexpr int Q1_REPL = 32;
static constexpr int Q1_FIELDS = 8;	/* cnt,qty,base,dcol,disc,+pad.. */
static constexpr int Q1_SLOTS = 6 * Q1_FIELDS;	/* 48 */
static constexpr int Q1_STRIDE = Q1_SLOTS + 1;	/* 49: odd → bank spread */

template <bool NT>
__device__ inline int64_t q1_ld64(const int64_t *p)
{
	return NT ? __builtin_nontemporal_load(p) : *p;
}

template <bool NT>
__global__ __launch_bounds__(THREADS, 2)
void k_q1_agg(const int32_t *__restrict__ shipdate,
	      const uint8_t *__restrict__ rflag,
	      const uint8_t *__restrict__ lstatus,
	      const int64_t *__restrict__ qty,
	      const int64_t *__restrict__ price,
	      const int64_t *__restrict__ disc,
	      const int64_t *__restrict__ tax,
	      int64_t n, int32_t cutoff, Q1DeviceAcc *acc)
{
	__shared__ unsigned long long lds[Q1_REPL * Q1_STRIDE];

	for (int i = threadIdx.x; i < Q1_REPL * Q1_STRIDE; i += blockDim.x)
		lds[i] = 0;
	__syncthreads();

	const int rep = threadIdx.x & (Q1_REPL - 1);
	unsigned long long *mine = &lds[rep * Q1_STRIDE];
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long bad = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int32_t sd = NT ? __builtin_nontemporal_load(&shipdate[i])
			: shipdate[i];

		if (sd > cutoff)	/* qual: l_shipdate <= cutoff */
			continue;
		{
			uint8_t rf = rflag[i];
			uint8_t ls = lstatus[i];
			int fi = (rf == 'N') ? 1 : ((rf == 'R') ? 2 : 0);
			int si = (ls == 'O') ? 1 : 0;

			bad |= (rf != 'A' && rf != 'N' && rf != 'R');
			bad |= (ls != 'F' && ls != 'O');
			{
				int g = (fi * 2 + si) * Q1_FIELDS;
				int64_t q = q1_ld64<NT>(&qty[i]);
				int64_t p = q1_ld64<NT>(&price[i]);
				int64_t d = q1_ld64<NT>(&disc[i]);
				int64_t t = q1_ld64<NT>(&tax[i]);
				/* mul_var exact: scale 2+2 then 4+2 */
				unsigned long long disc4 =
					(unsigned long long) (p * (100 - d));
				unsigned long long charge6 =
					disc4 * (unsigned long long) (100 + t);

				atomicAdd(&mine[g + 0], 1ull);
				atomicAdd(&mine[g + 1], (unsigned long long) q);
				atomicAdd(&mine[g + 2], (unsigned long long) p);
				atomicAdd(&mine[g + 3], (unsigned long long) d);
				atomicAdd(&mine[g + 4], disc4);
				atomicAdd(&mine[g + 5], charge6);
			}
		}
	}
	if (bad)
		atomicOr(&acc->err, 1ull);
	__syncthreads();

	/* flush: per-block sums fit u64 (DESIGN.md §overflow budget);
	 * 128-bit carry handled at the global accumulator */
	for (int slot = threadIdx.x; slot < Q1_SLOTS; slot += blockDim.x)
	{
		unsigned long long sum = 0;

		for (int r = 0; r < Q1_REPL; r++)
			sum += lds[r * Q1_STRIDE + slot];
		if (!sum)
			continue;
		{
			int g = slot / Q1_FIELDS;
			int f = slot % Q1_FIELDS;

			switch (f)
			{
				case 0: atomicAdd(&acc->v[g][0], sum); break;
				case 1: atomicAdd(&acc->v[g][1], sum); break;
				case 2: atomicAdd(&acc->v[g][2], sum); break;
				case 3: atomicAdd(&acc->v[g][3], sum); break;
				case 4:	/* disc4 int128: lo + carry */
				{
					unsigned long long old =
						atomicAdd(&acc->v[g][4], sum);
					if (old + sum < old)
						atomicAdd(&acc->v[g][5], 1ull);
					break;
				}
				case 5:	/* charge6 int128 */
				{
					unsigned long long old =
						atomicAdd(&acc->v[g][6], sum);
					if (old + sum < old)
						atomicAdd(&acc->v[g][7], 1ull);
					break;
				}
				default: break;
			}
		}
	}
}

hipError_t
launch_q1(hipStream_t s, const int32_t *shipdate, const uint8_t *rflag,
	  const uint8_t *lstatus, const int64_t *qty, const int64_t *price,
	  const int64_t *disc, const int64_t *tax, int64_t n, int32_t cutoff,
	  Q1DeviceAcc *acc)
{
	/* tuning knobs (benchmark sweeps; defaults are the shipped config) */
	int grid = grid_for(n);
	const char *gs = getenv("GG_Q1_GRID");
	/* nontemporal streaming loads measured +11%% on this kernel
	 * (6.38 vs 5.55 TB/s — tools/q1_sweep.py); default ON */
	const char *nts = getenv("GG_Q1_NT");
	bool nt = !(nts && nts[0] == '0');

	if (gs)
	{
		int64_t cap = (n + THREADS - 1) / THREADS;
		/* per-block partials are u64; rows-per-block × max charge6
		 * (~1.19e11, scale 6) must stay < 2^64 (DESIGN.md overflow
		 * budget), so a forced grid may not drop below this floor */
		int64_t floor_g = (int64_t) (((unsigned __int128) n *
					      120000000000ull) / ~0ull) + 1;
		int g = atoi(gs);

		if (g > 0)
		{
			if (g < floor_g)
				g = (int) floor_g;
			grid = (int) (g < cap ? g : cap);
		}
	}
	if (nt)
		hipLaunchKernelGGL(k_q1_agg<true>, dim3(grid), dim3(THREADS),
				   0, s, shipdate, rflag, lstatus, qty, price,
				   disc, tax, n, cutoff, acc);
	else
		hipLaunchKernelGGL(k_q1_agg<false>, dim3(grid), dim3(THREADS),
				   0, s, shipdate, rflag, lstatus, qty, price,
				   disc, tax, n, cutoff, acc);
	return hipGetLastError();
}

/* ------------------------------------------------------------------ */
/* Q1 over the packed companion (q1_pack.h): 12 B/row instead of 38    */
/* ------------------------------------------------------------------ */

typedef uint32_t q1_u32x4 __attribute__((ext_vector_type(4)));
typedef int32_t q1_i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long q1_u64x2 __attribute__((ext_vector_type(2)));
typedef long long q1_i64x2 __attribute__((ext_vector_type(2)));

static_assert(Q1P_THREADS == THREADS, "q1_pack.h sizes the grid for THREADS");

__device__ inline void
q1_pack_row(int32_t sd, uint8_t rf, uint8_t ls, int64_t q, int64_t p,
	    int64_t d, int64_t t, int32_t sd_base, unsigned long long *w8,
	    uint32_t *w4)
{
	int fi = (rf == 'A') ? 0 : ((rf == 'N') ? 1 : ((rf == 'R') ? 2 : -1));
	int si = (ls == 'F') ? 0 : ((ls == 'O') ? 1 : -1);
	uint32_t code = (fi < 0 || si < 0) ? Q1P_BAD_CODE
		: (uint32_t) (fi * 2 + si);

	/* the host proved every value inside its field (q1_pack_eligible) */
	*w8 = (unsigned long long) (uint32_t) p |
		((unsigned long long) ((uint32_t) q & 0xFFFFu) << 32) |
		((unsigned long long) ((uint32_t) d & 0xFFu) << 48) |
		((unsigned long long) ((uint32_t) t & 0xFFu) << 56);
	*w4 = (((uint32_t) sd - (uint32_t) sd_base) & 0xFFFFu) | (code << 16);
}

/* One lane packs 4 consecutive rows: eleven 16-byte-or-narrower loads of
 * the seven columns, three 16-byte stores.  Rows past the last whole quad
 * (n % 4) go one by one. */
__global__ __launch_bounds__(THREADS)
void k_q1_pack_build(const int32_t *__restrict__ shipdate,
		     const uint8_t *__restrict__ rflag,
		     const uint8_t *__restrict__ lstatus,
		     const int64_t *__restrict__ qty,
		     const int64_t *__restrict__ price,
		     const int64_t *__restrict__ disc,
		     const int64_t *__restrict__ tax,
		     int64_t n, int32_t sd_base,
		     unsigned long long *__restrict__ w8,
		     uint32_t *__restrict__ w4)
{
	const int64_t nq = n / Q1P_ROWS;
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	const int64_t gid = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;

	for (int64_t qd = gid; qd < nq; qd += stride)
	{
		const int64_t i = qd * Q1P_ROWS;
		q1_i32x4 sd = __builtin_nontemporal_load(
			(const q1_i32x4 *) &shipdate[i]);
		uint32_t rf = __builtin_nontemporal_load(
			(const uint32_t *) &rflag[i]);
		uint32_t ls = __builtin_nontemporal_load(
			(const uint32_t *) &lstatus[i]);
		q1_i64x2 q[2], p[2], d[2], t[2];
		unsigned long long o8[Q1P_ROWS];
		uint32_t o4[Q1P_ROWS];

#pragma unroll
		for (int h = 0; h < 2; h++)
		{
			q[h] = __builtin_nontemporal_load(
				(const q1_i64x2 *) &qty[i + 2 * h]);
			p[h] = __builtin_nontemporal_load(
				(const q1_i64x2 *) &price[i + 2 * h]);
			d[h] = __builtin_nontemporal_load(
				(const q1_i64x2 *) &disc[i + 2 * h]);
			t[h] = __builtin_nontemporal_load(
				(const q1_i64x2 *) &tax[i + 2 * h]);
		}
#pragma unroll
		for (int k = 0; k < Q1P_ROWS; k++)
			q1_pack_row(sd[k], (uint8_t) (rf >> (8 * k)),
				    (uint8_t) (ls >> (8 * k)), q[k >> 1][k & 1],
				    p[k >> 1][k & 1], d[k >> 1][k & 1],
				    t[k >> 1][k & 1], sd_base, &o8[k], &o4[k]);
		*(q1_u64x2 *) &w8[i] = q1_u64x2{o8[0], o8[1]};
		*(q1_u64x2 *) &w8[i + 2] = q1_u64x2{o8[2], o8[3]};
		*(q1_u32x4 *) &w4[i] = q1_u32x4{o4[0], o4[1], o4[2], o4[3]};
	}
	if (gid == 0)
		for (int64_t i = nq * Q1P_ROWS; i < n; i++)
			q1_pack_row(shipdate[i], rflag[i], lstatus[i], qty[i],
				    price[i], disc[i], tax[i], sd_base, &w8[i],
				    &w4[i]);
}

hipError_t
launch_q1_pack_build(hipStream_t s, const int32_t *shipdate,
		     const uint8_t *rflag, const uint8_t *lstatus,
		     const int64_t *qty, const int64_t *price,
		     const int64_t *disc, const int64_t *tax, int64_t n,
		     int32_t sd_base, unsigned long long *w8, uint32_t *w4)
{
	hipLaunchKernelGGL(k_q1_pack_build, dim3(grid_for(q1_pack_quads(n))),
			   dim3(THREADS), 0, s, shipdate, rflag, lstatus, qty,
			   price, disc, tax, n, sd_base, w8, w4);
	return hipGetLastError();
}

/* one row's terms, exact: disc4 < 2^39, charge6 < 2^48 */
struct Q1Terms
{
	unsigned long long cnt, q, p, d, disc4, charge6;
};

__device__ inline Q1Terms q1_unpack(unsigned long long w)
{
	Q1Terms r;

	r.cnt = 1;
	r.p = w & 0xFFFFFFFFull;
	r.q = (w >> 32) & 0xFFFFull;
	r.d = (w >> 48) & 0xFFull;
	r.disc4 = r.p * (100ull - r.d);
	r.charge6 = r.disc4 * (100ull + (w >> 56));
	return r;
}

__device__ inline void q1_add6(unsigned long long *mine, uint32_t code,
			       const Q1Terms &r)
{
	unsigned long long *g = &mine[code * Q1_FIELDS];

	atomicAdd(&g[0], r.cnt);
	atomicAdd(&g[1], r.q);
	atomicAdd(&g[2], r.p);
	atomicAdd(&g[3], r.d);
	atomicAdd(&g[4], r.disc4);
	atomicAdd(&g[5], r.charge6);
}

/*
 * Scan of the companion.  Each lane takes 4 consecutive rows per
 * iteration, so every load is 16 bytes and nontemporal: two of w8, one of
 * w4.  Accumulation is k_q1_agg's: six LDS adds per passing row into
 * replica lane % Q1_REPL.  At 12 B/row that still leaves the kernel at
 * the HBM limit; combining a lane's 4 rows first and 64 replicas were
 * measured and bought nothing (DESIGN.md "Packed Q1 companion").  A row
 * with the bad-flag code sets the error bit only if it passes the date
 * predicate, as in k_q1_agg.
 */
__global__ __launch_bounds__(THREADS, 2)
void k_q1_agg_packed(const unsigned long long *__restrict__ w8,
		     const uint32_t *__restrict__ w4, int64_t n, uint32_t c,
		     Q1DeviceAcc *acc)
{
	__shared__ unsigned long long lds[Q1_REPL * Q1_STRIDE];

	for (int i = threadIdx.x; i < Q1_REPL * Q1_STRIDE; i += blockDim.x)
		lds[i] = 0;
	__syncthreads();

	unsigned long long *mine =
		&lds[(threadIdx.x & (Q1_REPL - 1)) * Q1_STRIDE];
	const int64_t nq = n / Q1P_ROWS;
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	const int64_t gid = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	unsigned long long bad = 0;

	for (int64_t qd = gid; qd < nq; qd += stride)
	{
		q1_u32x4 f = __builtin_nontemporal_load(
			(const q1_u32x4 *) &w4[qd * Q1P_ROWS]);
		q1_u64x2 a = __builtin_nontemporal_load(
			(const q1_u64x2 *) &w8[qd * Q1P_ROWS]);
		q1_u64x2 b = __builtin_nontemporal_load(
			(const q1_u64x2 *) &w8[qd * Q1P_ROWS + 2]);
		unsigned long long w[Q1P_ROWS] = { a[0], a[1], b[0], b[1] };

#pragma unroll
		for (int k = 0; k < Q1P_ROWS; k++)
		{
			uint32_t code = (f[k] >> 16) & 7u;

			if ((f[k] & 0xFFFFu) > c)	/* l_shipdate <= cutoff */
				continue;
			if (code > 5u)
				bad = 1;
			else
				q1_add6(mine, code, q1_unpack(w[k]));
		}
	}
	/* the short tail (n % 4 rows, all of them when n < 4): scalar loads,
	 * nothing past row n - 1 is read */
	if (gid == 0)
		for (int64_t i = nq * Q1P_ROWS; i < n; i++)
		{
			uint32_t f = w4[i];
			uint32_t code = (f >> 16) & 7u;

			if ((f & 0xFFFFu) > c)
				continue;
			if (code > 5u)
				bad = 1;
			else
				q1_add6(mine, code, q1_unpack(w8[i]));
		}
	if (bad)
		atomicOr(&acc->err, 1ull);
	__syncthreads();

	/* flush as k_q1_agg does: per-block sums fit u64 (the host sizes the
	 * grid for it, q1_pack_grid), 128-bit carry at the global word */
	for (int slot = threadIdx.x; slot < Q1_SLOTS; slot += blockDim.x)
	{
		const int g = slot / Q1_FIELDS;
		const int fld = slot % Q1_FIELDS;
		unsigned long long sum = 0;

		if (fld > 5)
			continue;
		for (int r = 0; r < Q1_REPL; r++)
			sum += lds[r * Q1_STRIDE + slot];
		if (!sum)
			continue;
		if (fld < 4)
			atomicAdd(&acc->v[g][fld], sum);
		else
		{
			/* disc4 -> v[4], v[5]; charge6 -> v[6], v[7] */
			const int lo = fld == 4 ? 4 : 6;
			unsigned long long old = atomicAdd(&acc->v[g][lo], sum);

			if (old + sum < old)
				atomicAdd(&acc->v[g][lo + 1], 1ull);
		}
	}
}

hipError_t
launch_q1_packed(hipStream_t s, const unsigned long long *w8,
		 const uint32_t *w4, int64_t n, uint32_t c, uint64_t row_bound,
		 Q1DeviceAcc *acc)
{
	/* GG_Q1_GRID forces the grid as it does for k_q1_agg; the floor
	 * comes from this table's own maxima (q1_pack.h) */
	const char *gs = getenv("GG_Q1_GRID");
	int grid = (int) q1_pack_grid(n, gs ? atoi(gs) : 0, row_bound);

	hipLaunchKernelGGL(k_q1_agg_packed, dim3(grid), dim3(THREADS), 0, s,
			   w8, w4, n, c, acc);
	return hipGetLastError();
}

/* ------------------------------------------------------------------ */
/* Q1 over the 8 B/row tier of the companion (q1_pack.h)               */
/* ------------------------------------------------------------------ */

__device__ inline unsigned long long
q1_pack8_row(const Q1Pack8Layout &l, int32_t sd, uint8_t rf, uint8_t ls,
	     int64_t q, int64_t p, int64_t d, int64_t t, int32_t sd_base)
{
	int fi = (rf == 'A') ? 0 : ((rf == 'N') ? 1 : ((rf == 'R') ? 2 : -1));
	int si = (ls == 'F') ? 0 : ((ls == 'O') ? 1 : -1);
	uint32_t code = (fi < 0 || si < 0) ? Q1P_BAD_CODE
		: (uint32_t) (fi * 2 + si);

	return q1_pack8_word(l, (uint32_t) sd - (uint32_t) sd_base, code,
			     (uint32_t) d, (uint32_t) t, (uint32_t) q,
			     (uint32_t) p);
}

/* k_q1_pack_build for the 8 B tier: the same eleven loads per 4 rows, two
 * 16-byte stores. */
__global__ __launch_bounds__(THREADS)
void k_q1_pack8_build(const int32_t *__restrict__ shipdate,
		      const uint8_t *__restrict__ rflag,
		      const uint8_t *__restrict__ lstatus,
		      const int64_t *__restrict__ qty,
		      const int64_t *__restrict__ price,
		      const int64_t *__restrict__ disc,
		      const int64_t *__restrict__ tax,
		      int64_t n, int32_t sd_base, Q1Pack8Layout l,
		      unsigned long long *__restrict__ w)
{
	const int64_t nq = n / Q1P_ROWS;
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	const int64_t gid = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;

	for (int64_t qd = gid; qd < nq; qd += stride)
	{
		const int64_t i = qd * Q1P_ROWS;
		q1_i32x4 sd = __builtin_nontemporal_load(
			(const q1_i32x4 *) &shipdate[i]);
		uint32_t rf = __builtin_nontemporal_load(
			(const uint32_t *) &rflag[i]);
		uint32_t ls = __builtin_nontemporal_load(
			(const uint32_t *) &lstatus[i]);
		q1_i64x2 q[2], p[2], d[2], t[2];
		unsigned long long o[Q1P_ROWS];

#pragma unroll
		for (int h = 0; h < 2; h++)
		{
			q[h] = __builtin_nontemporal_load(
				(const q1_i64x2 *) &qty[i + 2 * h]);
			p[h] = __builtin_nontemporal_load(
				(const q1_i64x2 *) &price[i + 2 * h]);
			d[h] = __builtin_nontemporal_load(
				(const q1_i64x2 *) &disc[i + 2 * h]);
			t[h] = __builtin_nontemporal_load(
				(const q1_i64x2 *) &tax[i + 2 * h]);
		}
#pragma unroll
		for (int k = 0; k < Q1P_ROWS; k++)
			o[k] = q1_pack8_row(l, sd[k], (uint8_t) (rf >> (8 * k)),
					    (uint8_t) (ls >> (8 * k)),
					    q[k >> 1][k & 1], p[k >> 1][k & 1],
					    d[k >> 1][k & 1], t[k >> 1][k & 1],
					    sd_base);
		*(q1_u64x2 *) &w[i] = q1_u64x2{o[0], o[1]};
		*(q1_u64x2 *) &w[i + 2] = q1_u64x2{o[2], o[3]};
	}
	if (gid == 0)
		for (int64_t i = nq * Q1P_ROWS; i < n; i++)
			w[i] = q1_pack8_row(l, shipdate[i], rflag[i], lstatus[i],
					    qty[i], price[i], disc[i], tax[i],
					    sd_base);
}

hipError_t
launch_q1_pack8_build(hipStream_t s, const int32_t *shipdate,
		      const uint8_t *rflag, const uint8_t *lstatus,
		      const int64_t *qty, const int64_t *price,
		      const int64_t *disc, const int64_t *tax, int64_t n,
		      int32_t sd_base, const Q1Pack8Layout &l,
		      unsigned long long *w)
{
	hipLaunchKernelGGL(k_q1_pack8_build, dim3(grid_for(q1_pack_quads(n))),
			   dim3(THREADS), 0, s, shipdate, rflag, lstatus, qty,
			   price, disc, tax, n, sd_base, l, w);
	return hipGetLastError();
}

/* One row of the 8 B tier: the date predicate, then the bad-code rule of
 * k_q1_agg_packed, then the adds into the lane's replica.  price is a u32
 * (q1_pack_eligible), so disc4 is one 32x32->64 product and charge6 a
 * 64x32 one.  FOLD: count, sum(disc) and sum(qty) go into slot 0 as one
 * word (Q1Pack8Fold), four LDS adds instead of six. */
template <bool FOLD>
__device__ inline void
q1_row8(unsigned long long *mine, const Q1Pack8Layout &l,
	const Q1Pack8Fold &fo, uint32_t c, unsigned long long w,
	unsigned long long &bad)
{
	const uint32_t code = q1_pack8_code(l, w);

	if (q1_pack8_sd(l, w) > c)	/* l_shipdate <= cutoff */
		return;
	if (code > 5u)
	{
		bad = 1;
		return;
	}
	unsigned long long *g = &mine[code * Q1_FIELDS];
	const uint32_t d = q1_pack8_disc(l, w);
	const uint32_t t = q1_pack8_tax(l, w);
	const uint32_t q = q1_pack8_qty(l, w);
	const uint32_t p = q1_pack8_price(l, w);
	const unsigned long long disc4 = (unsigned long long) p * (100u - d);
	const unsigned long long charge6 = disc4 * (100u + t);

	if (FOLD)
		atomicAdd(&g[0], ((unsigned long long) q << 32) |
			  ((d << fo.d_shift) | 1u));
	else
	{
		atomicAdd(&g[0], 1ull);
		atomicAdd(&g[1], (unsigned long long) q);
		atomicAdd(&g[3], (unsigned long long) d);
	}
	atomicAdd(&g[2], (unsigned long long) p);
	atomicAdd(&g[4], disc4);
	atomicAdd(&g[5], charge6);
}

/*
 * Scan of the 8 B tier: k_q1_agg_packed with one array.  A lane takes 4
 * consecutive rows (a quad) through two 16-byte nontemporal loads, and two
 * of its quads per iteration with all four loads issued together: at
 * 8 B/row one quad per lane in flight no longer covers the HBM latency.
 * Which quads a lane takes is still the plain grid-stride assignment, so
 * q1_pack_rows_per_block and q1_pack_grid hold as they are.  The date
 * offset, the code and disc come out of a word's low dword.
 */
template <bool FOLD>
__global__ __launch_bounds__(THREADS, 2)
void k_q1_agg_packed8(const unsigned long long *__restrict__ wd, int64_t n,
		      uint32_t c, Q1Pack8Layout l, Q1Pack8Fold fo,
		      Q1DeviceAcc *acc)
{
	__shared__ unsigned long long lds[Q1_REPL * Q1_STRIDE];

	for (int i = threadIdx.x; i < Q1_REPL * Q1_STRIDE; i += blockDim.x)
		lds[i] = 0;
	__syncthreads();

	unsigned long long *mine =
		&lds[(threadIdx.x & (Q1_REPL - 1)) * Q1_STRIDE];
	const int64_t nq = n / Q1P_ROWS;
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	const int64_t gid = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	unsigned long long bad = 0;
	int64_t qd = gid;

	for (; qd + stride < nq; qd += 2 * stride)
	{
		const unsigned long long *r0 = &wd[qd * Q1P_ROWS];
		const unsigned long long *r1 = &wd[(qd + stride) * Q1P_ROWS];
		q1_u64x2 v[4] = {
			__builtin_nontemporal_load((const q1_u64x2 *) r0),
			__builtin_nontemporal_load((const q1_u64x2 *) (r0 + 2)),
			__builtin_nontemporal_load((const q1_u64x2 *) r1),
			__builtin_nontemporal_load((const q1_u64x2 *) (r1 + 2)),
		};

#pragma unroll
		for (int k = 0; k < 2 * Q1P_ROWS; k++)
			q1_row8<FOLD>(mine, l, fo, c, v[k >> 1][k & 1], bad);
	}
	if (qd < nq)		/* the lane's last quad, when it has an odd count */
	{
		const unsigned long long *r0 = &wd[qd * Q1P_ROWS];
		q1_u64x2 v[2] = {
			__builtin_nontemporal_load((const q1_u64x2 *) r0),
			__builtin_nontemporal_load((const q1_u64x2 *) (r0 + 2)),
		};

#pragma unroll
		for (int k = 0; k < Q1P_ROWS; k++)
			q1_row8<FOLD>(mine, l, fo, c, v[k >> 1][k & 1], bad);
	}
	/* the short tail (n % 4 rows): scalar loads in one thread, nothing
	 * past row n - 1 is read */
	if (gid == 0)
		for (int64_t i = nq * Q1P_ROWS; i < n; i++)
			q1_row8<FOLD>(mine, l, fo, c, wd[i], bad);
	if (bad)
		atomicOr(&acc->err, 1ull);
	__syncthreads();

	/* flush as k_q1_agg_packed does; a folded slot 0 is taken apart per
	 * replica, before the replicas are summed */
	for (int slot = threadIdx.x; slot < Q1_SLOTS; slot += blockDim.x)
	{
		const int g = slot / Q1_FIELDS;
		const int fld = slot % Q1_FIELDS;
		unsigned long long sum = 0;

		if (fld > 5)
			continue;
		if (FOLD && (fld == 0 || fld == 1 || fld == 3))
		{
			/* count | sum(disc) << d_shift | sum(qty) << 32 */
			const uint32_t sh = fld == 0 ? 0
				: (fld == 3 ? fo.d_shift : 32);
			const unsigned long long m = fld == 0
				? (1ull << fo.d_shift) - 1
				: (fld == 3 ? 0xFFFFFFFFull >> fo.d_shift
				   : 0xFFFFFFFFull);

#pragma unroll 1
			for (int r = 0; r < Q1_REPL; r++)
				sum += (lds[r * Q1_STRIDE + g * Q1_FIELDS] >> sh) & m;
		}
		else
			for (int r = 0; r < Q1_REPL; r++)
				sum += lds[r * Q1_STRIDE + slot];
		if (!sum)
			continue;
		if (fld < 4)
			atomicAdd(&acc->v[g][fld], sum);
		else
		{
			/* disc4 -> v[4], v[5]; charge6 -> v[6], v[7] */
			const int lo = fld == 4 ? 4 : 6;
			unsigned long long old = atomicAdd(&acc->v[g][lo], sum);

			if (old + sum < old)
				atomicAdd(&acc->v[g][lo + 1], 1ull);
		}
	}
}

hipError_t
launch_q1_packed8(hipStream_t s, const unsigned long long *w, int64_t n,
		  uint32_t c, uint64_t row_bound, const Q1Pack8Layout &l,
		  long long qmax, long long dmax, Q1DeviceAcc *acc)
{
	/* GG_Q1_GRID as for the 12 B tier; the fold is proven for the grid
	 * that runs, six adds otherwise */
	const char *gs = getenv("GG_Q1_GRID");
	int grid = (int) q1_pack_grid(n, gs ? atoi(gs) : 0, row_bound);
	Q1Pack8Fold fo = q1_pack8_fold(n, grid, qmax, dmax);

	if (fo.on)
		hipLaunchKernelGGL(k_q1_agg_packed8<true>, dim3(grid),
				   dim3(THREADS), 0, s, w, n, c, l, fo, acc);
	else
		hipLaunchKernelGGL(k_q1_agg_packed8<false>, dim3(grid),
				   dim3(THREADS), 0, s, w, n, c, l, fo, acc);
	return hipGetLastError();
}

/* ------------------------------------------------------------------ */
/* BASELINE config 1: sum(l_extendedprice) where l_shipdate < cutoff   */
/* ------------------------------------------------------------------ */

__global__ __launch_bounds__(THREADS, 2)
void k_sumprice(const int32_t *__restrict__ shipdate,
		const int64_t *__restrict__ price, int64_t n, int32_t cutoff,
		SumPriceAcc *acc)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long sum = 0, cnt = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
		if (nt_ld32(&shipdate[i]) < cutoff)
		{
			sum += (unsigned long long) nt_ld64(&price[i]);
			cnt++;
		}
	/* block-level reduction: one atomic pair per block (per-wave
	 * flushes serialize at the ~88 atomics/µs hot-word wall) */
	__shared__ unsigned long long ls[4][2];

	for (int off = 32; off; off >>= 1)
	{
		sum += __shfl_down(sum, off, 64);
		cnt += __shfl_down(cnt, off, 64);
	}
	if ((threadIdx.x & 63) == 0)
	{
		ls[threadIdx.x >> 6][0] = sum;
		ls[threadIdx.x >> 6][1] = cnt;
	}
	__syncthreads();
	if (threadIdx.x == 0)
	{
		unsigned long long s = 0, c = 0;

		for (int i = 0; i < (int) (blockDim.x >> 6); i++)
		{
			s += ls[i][0];
			c += ls[i][1];
		}
		if (s || c)
		{
			atomicAdd(&acc->sum_c, s);
			atomicAdd(&acc->count, c);
		}
	}
}

hipError_t
launch_sumprice(hipStream_t s, const int32_t *shipdate, const int64_t *price,
		int64_t n, int32_t cutoff, SumPriceAcc *acc)
{
	hipLaunchKernelGGL(k_sumprice, dim3(grid_for(n)), dim3(THREADS), 0, s,
			   shipdate, price, n, cutoff, acc);
	return hipGetLastError();
}

/* ------------------------------------------------------------------ */
/* synthetic generation (gg_gen.h, shared with the CPU oracle)         */
/* ------------------------------------------------------------------ */

/* which_table for shard counting */
enum { TAB_LI = 0, TAB_ORD = 1, TAB_CUST = 2 };

__device__ inline int
li_seg(uint64_t /*seed*/, int64_t row, int nseg)
{
	int64_t orderkey = (row >> 2) + 1;

	return gg_cdbhash_segment_int8(orderkey, nseg);
}

__global__ void
k_count_shard(int64_t row_lo, int64_t n, int nseg, int seg, int which,
	      uint64_t seed, int64_t sf, unsigned long long *out_count)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long c = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t row = row_lo + i;
		int s;

		if (which == TAB_LI)
			s = li_seg(seed, row, nseg);
		else	/* orders / customer: key = row+1 (dense) */
			s = gg_cdbhash_segment_int8(row + 1, nseg);
		if (s == seg)
			c++;
	}
	for (int off = 32; off; off >>= 1)
		c += __shfl_down(c, off, 64);
	if ((threadIdx.x & 63) == 0)
		atomicAdd(out_count, c);
}

hipError_t
launch_count_shard(hipStream_t s, int64_t row_lo, int64_t n, int nseg,
		   int seg, int which_table, uint64_t seed, int64_t sf,
		   unsigned long long *out_count)
{
	hipLaunchKernelGGL(k_count_shard, dim3(grid_for(n)), dim3(THREADS), 0,
			   s, row_lo, n, nseg, seg, which_table, seed, sf,
			   out_count);
	return hipGetLastError();
}

__global__ void
k_gen_lineitem(uint64_t seed, int64_t sf, int64_t row_lo, int64_t n,
	       int nseg, int seg,
	       int64_t *__restrict__ orderkey, int64_t *__restrict__ qty,
	       int64_t *__restrict__ price, int64_t *__restrict__ disc,
	       int64_t *__restrict__ tax, int32_t *__restrict__ shipdate,
	       uint8_t *__restrict__ rflag, uint8_t *__restrict__ lstatus,
	       int64_t *__restrict__ suppkey, unsigned long long *out_count)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t row = row_lo + i;
		bool own = (nseg <= 1) || (li_seg(seed, row, nseg) == seg);
		int64_t idx;

		if (nseg <= 1)
			idx = i;
		else
		{
			/* wave-aggregated append (Guideline 12) */
			unsigned long long mask = __ballot(own);
			int lane = threadIdx.x & 63;
			int nbefore = __popcll(mask & ((1ull << lane) - 1));
			int total = __popcll(mask);
			int leader = __ffsll((long long) mask) - 1;
			unsigned long long base = 0;

			if (total && lane == leader)
				base = atomicAdd(out_count,
						 (unsigned long long) total);
			if (total)
				base = __shfl(base, leader, 64);
			idx = (int64_t) (base + (unsigned) nbefore);
		}
		if (!own)
			continue;
		{
			gg_lineitem_row r;

			gg_gen_lineitem(seed, row, &r);
			orderkey[idx] = r.l_orderkey;
			qty[idx] = r.l_quantity_c;
			price[idx] = r.l_extendedprice_c;
			disc[idx] = r.l_discount_c;
			tax[idx] = r.l_tax_c;
			shipdate[idx] = r.l_shipdate;
			rflag[idx] = r.l_returnflag;
			lstatus[idx] = r.l_linestatus;
			suppkey[idx] = gg_l_suppkey(seed, row, sf);
		}
	}
}

hipError_t
launch_gen_lineitem(hipStream_t s, uint64_t seed, int64_t sf, int64_t row_lo,
		    int64_t n, int nseg, int seg, int64_t *orderkey,
		    int64_t *qty, int64_t *price, int64_t *disc, int64_t *tax,
		    int32_t *shipdate, uint8_t *rflag, uint8_t *lstatus,
		    int64_t *suppkey, unsigned long long *out_count)
{
	hipLaunchKernelGGL(k_gen_lineitem, dim3(grid_for(n)), dim3(THREADS),
			   0, s, seed, sf, row_lo, n, nseg, seg, orderkey,
			   qty, price, disc, tax, shipdate, rflag, lstatus,
			   suppkey, out_count);
	return hipGetLastError();
}

__global__ void
k_gen_orders(uint64_t seed, int64_t sf, int64_t row_lo, int64_t n, int nseg,
	     int seg, int64_t *__restrict__ orderkey,
	     int64_t *__restrict__ custkey, int32_t *__restrict__ orderdate,
	     int32_t *__restrict__ prio, unsigned long long *out_count)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t okey = row_lo + i + 1;
		bool own = (nseg <= 1) ||
			(gg_cdbhash_segment_int8(okey, nseg) == seg);
		int64_t idx = i;

		if (nseg > 1)
		{
			unsigned long long mask = __ballot(own);
			int lane = threadIdx.x & 63;
			int nbefore = __popcll(mask & ((1ull << lane) - 1));
			int total = __popcll(mask);
			int leader = __ffsll((long long) mask) - 1;
			unsigned long long base = 0;

			if (total && lane == leader)
				base = atomicAdd(out_count,
						 (unsigned long long) total);
			if (total)
				base = __shfl(base, leader, 64);
			idx = (int64_t) (base + (unsigned) nbefore);
		}
		if (!own)
			continue;
		orderkey[idx] = okey;
		custkey[idx] = gg_o_custkey(seed, okey, sf);
		orderdate[idx] = gg_o_orderdate(seed, okey);
		prio[idx] = gg_o_shippriority(seed, okey);
	}
}

hipError_t
launch_gen_orders(hipStream_t s, uint64_t seed, int64_t sf, int64_t row_lo,
		  int64_t n, int nseg, int seg, int64_t *orderkey,
		  int64_t *custkey, int32_t *orderdate, int32_t *prio,
		  unsigned long long *out_count)
{
	hipLaunchKernelGGL(k_gen_orders, dim3(grid_for(n)), dim3(THREADS), 0,
			   s, seed, sf, row_lo, n, nseg, seg, orderkey,
			   custkey, orderdate, prio, out_count);
	return hipGetLastError();
}

__global__ void
k_gen_customer(uint64_t seed, int64_t row_lo, int64_t n, int nseg, int seg,
	       int64_t *__restrict__ custkey, uint8_t *__restrict__ mktseg,
	       uint8_t *__restrict__ nationkey, unsigned long long *out_count)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t ckey = row_lo + i + 1;
		bool own = (nseg <= 1) ||
			(gg_cdbhash_segment_int8(ckey, nseg) == seg);
		int64_t idx = i;

		if (nseg > 1)
		{
			unsigned long long mask = __ballot(own);
			int lane = threadIdx.x & 63;
			int nbefore = __popcll(mask & ((1ull << lane) - 1));
			int total = __popcll(mask);
			int leader = __ffsll((long long) mask) - 1;
			unsigned long long base = 0;

			if (total && lane == leader)
				base = atomicAdd(out_count,
						 (unsigned long long) total);
			if (total)
				base = __shfl(base, leader, 64);
			idx = (int64_t) (base + (unsigned) nbefore);
		}
		if (!own)
			continue;
		custkey[idx] = ckey;
		mktseg[idx] = gg_c_mktsegment(seed, ckey);
		nationkey[idx] = gg_c_nationkey(seed, ckey);
	}
}

hipError_t
launch_gen_customer(hipStream_t s, uint64_t seed, int64_t row_lo, int64_t n,
		    int nseg, int seg, int64_t *custkey, uint8_t *mktseg,
		    uint8_t *nationkey, unsigned long long *out_count)
{
	hipLaunchKernelGGL(k_gen_customer, dim3(grid_for(n)), dim3(THREADS),
			   0, s, seed, row_lo, n, nseg, seg, custkey, mktseg,
			   nationkey, out_count);
	return hipGetLastError();
}


/* wave-aggregated append: one returning atomicAdd per wave instead of
 * per lane (a single shared counter saturates at ~88 returning
 * atomics/us — MI355X_MICROARCH "dequeue" row; per-lane appends made a
 * 14.6M-row compaction 10x slower than the work itself) */
__device__ inline unsigned long long
wave_append(unsigned long long *ctr, bool take)
{
	unsigned long long mask = __ballot(take);
	int lane = (int) (threadIdx.x & 63);
	unsigned long long base = 0;

	if (mask)
	{
		int leader = __ffsll((long long) mask) - 1;

		if (lane == leader)
			base = atomicAdd(ctr,
					 (unsigned long long) __popcll(mask));
		base = __shfl(base, leader, 64);
	}
	return base + (unsigned long long) __popcll(mask &
						    ((1ull << lane) - 1));
}


/* Block-claimed compaction: pass 1 counts the block's survivors
 * (registers + one wave/LDS reduction), thread 0 claims ONE
 * contiguous region from the global counter, pass 2 appends through
 * an LDS cursor.  Even the wave-aggregated global append serializes
 * at the ~88 returning-atomics/µs hot-word wall (~10 ms per 57M-row
 * compaction); this makes it 2048 global atomics total.  Output
 * order within the region is block-local — all consumers on this
 * path are order-insensitive (aggregates / unique-key stores). */
__device__ inline unsigned long long
block_claim(unsigned long long *lds4, unsigned long long *bbase,
	    unsigned long long my, unsigned long long *global_ctr)
{
	for (int off = 32; off; off >>= 1)
		my += __shfl_down(my, off, 64);
	if ((threadIdx.x & 63) == 0)
		lds4[threadIdx.x >> 6] = my;
	__syncthreads();
	if (threadIdx.x == 0)
	{
		unsigned long long t = 0;

		for (int i = 0; i < (int) (blockDim.x >> 6); i++)
			t += lds4[i];
		*bbase = t ? atomicAdd(global_ctr, t) : 0;
	}
	__syncthreads();
	return *bbase;
}

/* ------------------------------------------------------------------ */
/* hash join build/probe (open addressing, key 0 = empty)              */
/* ------------------------------------------------------------------ */

__device__ inline uint64_t
ht_start(int64_t key, uint64_t nslots)
{
	return (uint64_t) gg_hashint8(key) & (nslots - 1);
}

/* blocked Bloom: one word per key, two bits derived from a remix of the
 * same 32-bit hash; one memory access per membership test */
__device__ inline unsigned long long
bloom_mask(uint32_t h, uint64_t words, uint64_t *word_idx)
{
	uint32_t h2 = h * 0x9E3779B1u;

	*word_idx = (uint64_t) (h >> 6) & (words - 1);
	return (1ull << (h2 & 63)) | (1ull << ((h2 >> 6) & 63));
}

__device__ inline void
bloom_insert(unsigned long long *bloom, uint64_t words, int64_t key)
{
	uint64_t w;
	unsigned long long m = bloom_mask(gg_hashint8(key), words, &w);

	atomicOr(&bloom[w], m);
}

__device__ inline bool
bloom_maybe(const unsigned long long *__restrict__ bloom, uint64_t words,
	    uint32_t h)
{
	uint64_t w;
	unsigned long long m = bloom_mask(h, words, &w);

	return (bloom[w] & m) == m;
}

/* insert key into a set (customer build side, nodeHash.c:905) */
__global__ void
k_build_set(const int64_t *__restrict__ keys,
	    const uint8_t *__restrict__ filter_col, uint8_t filter_val,
	    int64_t n, unsigned long long *__restrict__ tkeys,
	    uint64_t nslots, unsigned long long *__restrict__ bloom,
	    uint64_t bwords)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t k;
		uint64_t pos;

		if (filter_col && filter_col[i] != filter_val)
			continue;
		k = keys[i];
		if (bloom)
			bloom_insert(bloom, bwords, k);
		pos = ht_start(k, nslots);
		for (;;)
		{
			unsigned long long prev =
				atomicCAS(&tkeys[pos], 0ull,
					  (unsigned long long) k);
			if (prev == 0 || prev == (unsigned long long) k)
				break;
			pos = (pos + 1) & (nslots - 1);
		}
	}
}

hipError_t
launch_build_set(hipStream_t s, const int64_t *keys,
		 const uint8_t *filter_col, uint8_t filter_val, int64_t n,
		 DeviceHashTable t)
{
	hipLaunchKernelGGL(k_build_set, dim3(grid_for(n)), dim3(THREADS), 0,
			   s, keys, filter_col, filter_val, n, t.keys,
			   t.nslots, t.bloom, t.bloom_words);
	return hipGetLastError();
}

__device__ inline bool
ht_contains_b(const unsigned long long *__restrict__ tkeys, uint64_t nslots,
	      const unsigned long long *__restrict__ bloom, uint64_t bwords,
	      int64_t key)
{
	uint32_t h = gg_hashint8(key);

	if (bloom && !bloom_maybe(bloom, bwords, h))
		return false;
	{
		uint64_t pos = (uint64_t) h & (nslots - 1);

		for (;;)
		{
			unsigned long long v = tkeys[pos];

			if (v == (unsigned long long) key)
				return true;
			if (v == 0)
				return false;
			pos = (pos + 1) & (nslots - 1);
		}
	}
}

__device__ inline bool
ht_contains(const unsigned long long *__restrict__ tkeys, uint64_t nslots,
	    int64_t key)
{
	uint64_t pos = ht_start(key, nslots);

	for (;;)
	{
		unsigned long long v = tkeys[pos];

		if (v == (unsigned long long) key)
			return true;
		if (v == 0)
			return false;
		pos = (pos + 1) & (nslots - 1);
	}
}

/* orders: filter date, probe customer set, insert (okey → date|prio)
 * — the build side of the o⋈l join (nodeHashjoin state machine
 * HJ_BUILD_HASHTABLE, nodeHash.c:88–176) fused with the c⋈o probe */
__global__ void
k_build_orders(const int64_t *__restrict__ okey,
	       const int64_t *__restrict__ ckey,
	       const int32_t *__restrict__ odate,
	       const int32_t *__restrict__ prio, int64_t n, int32_t cutoff,
	       const unsigned long long *__restrict__ cust_keys,
	       uint64_t cust_slots,
	       const unsigned long long *__restrict__ cust_bloom,
	       uint64_t cust_bwords,
	       const unsigned long long *__restrict__ cust_bits,
	       int64_t cust_dlen,
	       unsigned long long *__restrict__ tkeys,
	       unsigned long long *__restrict__ tpayload, uint64_t nslots,
	       unsigned long long *__restrict__ bloom, uint64_t bwords,
	       unsigned long long *match_count)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long matches = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		/* dense loads: at ~46% date selectivity a masked load
		 * touches nearly every line anyway, so load all three
		 * streams coalesced and filter afterwards */
		int32_t d = nt_ld32(&odate[i]);
		int64_t ck = nt_ld64(&ckey[i]);
		int64_t k = nt_ld64(&okey[i]);

		if (d >= cutoff)	/* qual: o_orderdate < cutoff */
			continue;
		if (cust_bits)
		{
			if (ck < 0 || ck >= cust_dlen ||
			    !((cust_bits[ck >> 6] >> (ck & 63)) & 1))
				continue;
		}
		else if (!ht_contains_b(cust_keys, cust_slots, cust_bloom,
					cust_bwords, ck))
			continue;
		matches++;
		{
			uint64_t pos = ht_start(k, nslots);

			if (bloom)
				bloom_insert(bloom, bwords, k);
			unsigned long long pay =
				(unsigned long long) (uint32_t) odate[i] |
				((unsigned long long) (uint32_t) prio[i] << 32);

			for (;;)
			{
				unsigned long long prev =
					atomicCAS(&tkeys[pos], 0ull,
						  (unsigned long long) k);
				if (prev == 0)
				{
					tpayload[pos] = pay;
					break;
				}
				if (prev == (unsigned long long) k)
					break;	/* PK: cannot happen */
				pos = (pos + 1) & (nslots - 1);
			}
		}
	}
	for (int off = 32; off; off >>= 1)
		matches += __shfl_down(matches, off, 64);
	if ((threadIdx.x & 63) == 0 && matches)
		atomicAdd(match_count, matches);
}

hipError_t
launch_build_orders(hipStream_t s, const int64_t *okey, const int64_t *ckey,
		    const int32_t *odate, const int32_t *prio, int64_t n,
		    int32_t cutoff, DeviceHashTable cust,
		    const unsigned long long *cust_bits, int64_t cust_dlen,
		    DeviceHashTable ord, unsigned long long *match_count)
{
	hipLaunchKernelGGL(k_build_orders, dim3(grid_for(n)), dim3(THREADS),
			   0, s, okey, ckey, odate, prio, n, cutoff,
			   cust.keys, cust.nslots, cust.bloom,
			   cust.bloom_words, cust_bits, cust_dlen,
			   ord.keys, ord.payload,
			   ord.nslots, ord.bloom, ord.bloom_words,
			   match_count);
	return hipGetLastError();
}

/* count-only variants used to size the tables exactly (two-phase;
 * ExecChooseHashTableSize analog, nodeHash.c:450) */
__global__ void
k_count_filter_u8(const uint8_t *__restrict__ col, uint8_t val, int64_t n,
		  unsigned long long *out)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long c = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
		c += (col[i] == val);
	for (int off = 32; off; off >>= 1)
		c += __shfl_down(c, off, 64);
	if ((threadIdx.x & 63) == 0 && c)
		atomicAdd(out, c);
}

__global__ void
k_count_orders_match(const int64_t *__restrict__ ckey,
		     const int32_t *__restrict__ odate, int64_t n,
		     int32_t cutoff,
		     const unsigned long long *__restrict__ cust_keys,
		     uint64_t cust_slots,
		     const unsigned long long *__restrict__ cust_bloom,
		     uint64_t cust_bwords,
		     const unsigned long long *__restrict__ cust_bits,
		     int64_t cust_dlen, unsigned long long *out)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long c = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		if (odate[i] >= cutoff)
			continue;
		if (cust_bits)
		{
			int64_t ck = ckey[i];

			c += (ck >= 0 && ck < cust_dlen &&
			      ((cust_bits[ck >> 6] >> (ck & 63)) & 1));
		}
		else
			c += ht_contains_b(cust_keys, cust_slots, cust_bloom,
					   cust_bwords, ckey[i]);
	}
	for (int off = 32; off; off >>= 1)
		c += __shfl_down(c, off, 64);
	if ((threadIdx.x & 63) == 0 && c)
		atomicAdd(out, c);
}

/* lineitem probe + revenue aggregation into the order slot — the probe
 * loop (nodeHash.c:1163 ExecScanHashBucket) fused with the group-by
 * transition (group key l_orderkey ≡ join key, so the matched order's
 * slot IS the group slot; execHHashagg.c:456 lookup + nodeAgg advance) */
__global__ __launch_bounds__(THREADS, 2)
void k_probe_lineitem(const int64_t *__restrict__ okey,
		      const int32_t *__restrict__ shipdate,
		      const int64_t *__restrict__ price,
		      const int64_t *__restrict__ disc, int64_t n,
		      int32_t cutoff,
		      const unsigned long long *__restrict__ tkeys,
		      unsigned long long *__restrict__ trev, uint64_t nslots,
		      const unsigned long long *__restrict__ bloom,
		      uint64_t bwords, unsigned long long *join_rows)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long joined = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		/* dense loads (54% date selectivity): shipdate + okey
		 * coalesced, then Bloom before any table access */
		int32_t sd = nt_ld32(&shipdate[i]);
		int64_t k = nt_ld64(&okey[i]);

		if (sd <= cutoff)	/* qual: l_shipdate > cutoff */
			continue;
		{
			uint32_t h = gg_hashint8(k);
			uint64_t pos;

			if (bloom && !bloom_maybe(bloom, bwords, h))
				continue;
			pos = (uint64_t) h & (nslots - 1);
			for (;;)
			{
				unsigned long long v = tkeys[pos];

				if (v == 0)
					break;	/* miss */
				if (v == (unsigned long long) k)
				{
					unsigned long long rev4 =
						(unsigned long long)
						(price[i] * (100 - disc[i]));
					atomicAdd(&trev[pos], rev4);
					joined++;
					break;
				}
				pos = (pos + 1) & (nslots - 1);
			}
		}
	}
	for (int off = 32; off; off >>= 1)
		joined += __shfl_down(joined, off, 64);
	if ((threadIdx.x & 63) == 0 && joined)
		atomicAdd(join_rows, joined);
}

hipError_t
launch_probe_lineitem(hipStream_t s, const int64_t *okey,
		      const int32_t *shipdate, const int64_t *price,
		      const int64_t *disc, int64_t n, int32_t cutoff,
		      DeviceHashTable ord, unsigned long long *join_rows)
{
	hipLaunchKernelGGL(k_probe_lineitem, dim3(grid_for(n)), dim3(THREADS),
			   0, s, okey, shipdate, price, disc, n, cutoff,
			   ord.keys, ord.rev, ord.nslots, ord.bloom,
			   ord.bloom_words, join_rows);
	return hipGetLastError();
}

/* ------------------------------------------------------------------ */
/* Q3 result extraction: stats, max, histogram-select, collect         */
/* ------------------------------------------------------------------ */

/* one pass: group count, int128 revenue sum, checksum AND max revenue
 * (out5 = {ng, rev_lo, rev_carry, checksum, max_rev}) */
__global__ void
k_q3_stats(const unsigned long long *__restrict__ tkeys,
	   const unsigned long long *__restrict__ tpayload,
	   const unsigned long long *__restrict__ trev, uint64_t nslots,
	   unsigned long long *out5)
{
	const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
	unsigned long long ng = 0, rev = 0, carry = 0, ck = 0, mx = 0;

	for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < nslots; i += stride)
	{
		unsigned long long k = tkeys[i];
		unsigned long long r;

		if (!k)
			continue;
		r = trev[i];
		if (!r)
			continue;	/* order matched but no lines joined */
		ng++;
		mx = max(mx, r);
		{
			unsigned long long old = rev;

			rev += r;
			carry += (rev < old);
		}
		{
			unsigned long long pay = tpayload[i];
			int32_t date = (int32_t) (uint32_t) pay;
			int32_t prio = (int32_t) (uint32_t) (pay >> 32);

			ck += gg_group_hash((int64_t) k, r, 0, date, prio);
		}
	}
	for (int off = 32; off; off >>= 1)
	{
		unsigned long long orev = rev;

		ng += __shfl_down(ng, off, 64);
		rev += __shfl_down(rev, off, 64);
		carry += __shfl_down(carry, off, 64) + (rev < orev);
		ck += __shfl_down(ck, off, 64);
		mx = max(mx, __shfl_down(mx, off, 64));
	}
	if ((threadIdx.x & 63) == 0 && ng)
	{
		atomicAdd(&out5[0], ng);
		{
			unsigned long long old = atomicAdd(&out5[1], rev);

			if (old + rev < old)
				atomicAdd(&out5[2], 1ull);
			atomicAdd(&out5[2], carry);
		}
		atomicAdd(&out5[3], ck);
		atomicMax(&out5[4], mx);
	}
}

hipError_t
launch_q3_stats(hipStream_t s, DeviceHashTable ord, unsigned long long *out5)
{
	hipLaunchKernelGGL(k_q3_stats, dim3(grid_for((int64_t) ord.nslots)),
			   dim3(THREADS), 0, s, ord.keys, ord.payload,
			   ord.rev, ord.nslots, out5);
	return hipGetLastError();
}

__device__ inline int
q3_shift_for(unsigned long long maxrev)
{
	int shift = 0;

	while ((maxrev >> shift) > 65535)
		shift++;
	return shift;
}

__global__ void
k_q3_hist(const unsigned long long *__restrict__ tkeys,
	  const unsigned long long *__restrict__ trev, uint64_t nslots,
	  const unsigned long long *__restrict__ stats5,
	  unsigned int *__restrict__ hist64k)
{
	const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
	const int shift = q3_shift_for(stats5[4]);

	for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < nslots; i += stride)
	{
		unsigned long long r;

		if (!tkeys[i])
			continue;
		r = trev[i];
		if (!r)
			continue;
		{
			unsigned long long bin = r >> shift;

			if (bin > 65535)
				bin = 65535;
			atomicAdd(&hist64k[bin], 1u);
		}
	}
}

hipError_t
launch_q3_hist(hipStream_t s, DeviceHashTable ord,
	       const unsigned long long *stats5, unsigned int *hist64k)
{
	hipLaunchKernelGGL(k_q3_hist, dim3(grid_for((int64_t) ord.nslots)),
			   dim3(THREADS), 0, s, ord.keys, ord.rev, ord.nslots,
			   stats5, hist64k);
	return hipGetLastError();
}

/* one block: walk the histogram from the top bin until >= k candidates;
 * emit the revenue threshold (device-side — no host round trip) */
__global__ __launch_bounds__(1024)
void k_q3_threshold(const unsigned int *__restrict__ hist64k,
		    const unsigned long long *__restrict__ stats5, int64_t k,
		    unsigned long long *__restrict__ out_thr)
{
	__shared__ unsigned long long partial[1024];

	/* each thread sums its 64-bin chunk (chunk 1023 = highest bins) */
	unsigned long long s = 0;

	for (int b = 0; b < 64; b++)
		s += hist64k[threadIdx.x * 64 + b];
	partial[threadIdx.x] = s;
	__syncthreads();
	if (threadIdx.x == 0)
	{
		unsigned long long cum = 0;
		int chunk = 1023;

		for (; chunk > 0; chunk--)
		{
			if (cum + partial[chunk] >= (unsigned long long) k)
				break;
			cum += partial[chunk];
		}
		{
			unsigned long long bin = (unsigned long long) chunk * 64 + 63;
			int b = 63;

			for (; b > 0; b--)
			{
				unsigned long long c =
					hist64k[chunk * 64 + b];

				if (cum + c >= (unsigned long long) k)
					break;
				cum += c;
			}
			bin = (unsigned long long) chunk * 64 + b;
			{
				int shift = q3_shift_for(stats5[4]);
				unsigned long long thr = bin << shift;

				*out_thr = thr ? thr : 1;
			}
		}
	}
}

hipError_t
launch_q3_threshold(hipStream_t s, const unsigned int *hist64k,
		    const unsigned long long *stats5, int64_t k,
		    unsigned long long *out_thr)
{
	hipLaunchKernelGGL(k_q3_threshold, dim3(1), dim3(1024), 0, s,
			   hist64k, stats5, k, out_thr);
	return hipGetLastError();
}

__global__ void
k_q3_collect(const unsigned long long *__restrict__ tkeys,
	     const unsigned long long *__restrict__ tpayload,
	     const unsigned long long *__restrict__ trev, uint64_t nslots,
	     const unsigned long long *__restrict__ thr_ptr,
	     gg_q3_result_row *__restrict__ out,
	     unsigned long long *out_count, uint64_t cap)
{
	const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
	const unsigned long long threshold = *thr_ptr;

	for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < nslots; i += stride)
	{
		unsigned long long k = tkeys[i];
		unsigned long long r = k ? trev[i] : 0;
		bool take = (k && r && r >= threshold);
		unsigned long long idx = wave_append(out_count, take);

		if (!take || idx >= cap)
			continue;
		{
			unsigned long long pay = tpayload[i];

			out[idx].orderkey = (int64_t) k;
			out[idx].rev_lo = r;
			out[idx].rev_hi = 0;
			out[idx].orderdate = (int32_t) (uint32_t) pay;
			out[idx].shippriority =
				(int32_t) (uint32_t) (pay >> 32);
		}
	}
}

hipError_t
launch_q3_collect(hipStream_t s, DeviceHashTable ord,
		  const unsigned long long *thr_ptr, gg_q3_result_row *out,
		  unsigned long long *out_count, uint64_t cap)
{
	hipLaunchKernelGGL(k_q3_collect, dim3(grid_for((int64_t) ord.nslots)),
			   dim3(THREADS), 0, s, ord.keys, ord.payload,
			   ord.rev, ord.nslots, thr_ptr, out, out_count,
			   cap);
	return hipGetLastError();
}

/* ------------------------------------------------------------------ */
/* Motion partition (redistribute routing, nodeMotion.c:1600–1636)     */
/* ------------------------------------------------------------------ */

__global__ void
k_part_count(const int64_t *__restrict__ key, int64_t n, int nseg,
	     unsigned long long *__restrict__ counts)
{
	/* per-row global atomics on <= nseg words serialize at the
	 * ~88 atomics/µs hot-word wall (650 ms measured at 57M rows,
	 * nseg=1): count in LDS, flush once per block per dest */
	__shared__ unsigned long long lcnt[64];

	for (int d = threadIdx.x; d < nseg; d += blockDim.x)
		lcnt[d] = 0;
	__syncthreads();

	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
		atomicAdd(&lcnt[gg_cdbhash_segment_int8(key[i], nseg)],
			  1ull);
	__syncthreads();
	for (int d = threadIdx.x; d < nseg; d += blockDim.x)
		if (lcnt[d])
			atomicAdd(&counts[d], lcnt[d]);
}

hipError_t
launch_part_count(hipStream_t s, const int64_t *key, int64_t n, int nseg,
		  unsigned long long *counts)
{
	if (nseg > 64)
		return hipErrorInvalidValue;	/* LDS count array bound */
	hipLaunchKernelGGL(k_part_count, dim3(grid_for(n)), dim3(THREADS), 0,
			   s, key, n, nseg, counts);
	return hipGetLastError();
}

__global__ void
k_part_scatter3(const int64_t *__restrict__ key, int64_t n, int nseg,
		const int64_t *__restrict__ a, const int64_t *__restrict__ b,
		const int64_t *__restrict__ c,
		unsigned long long *__restrict__ offsets,
		int64_t *__restrict__ oa, int64_t *__restrict__ ob,
		int64_t *__restrict__ oc)
{
	/* two passes: count the block's rows per dest in LDS, claim one
	 * contiguous region per (block, dest) with a single global
	 * atomic each, then append through LDS cursors — per-row
	 * returning atomics on nseg hot words measured 650 ms at 57M
	 * rows (the ~88 atomics/µs wall) */
	__shared__ unsigned long long lcnt[64], lbase[64];

	for (int d = threadIdx.x; d < nseg; d += blockDim.x)
		lcnt[d] = 0;
	__syncthreads();

	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
		atomicAdd(&lcnt[gg_cdbhash_segment_int8(key[i], nseg)], 1ull);
	__syncthreads();
	for (int d = threadIdx.x; d < nseg; d += blockDim.x)
	{
		lbase[d] = lcnt[d] ? atomicAdd(&offsets[d], lcnt[d]) : 0;
		lcnt[d] = 0;
	}
	__syncthreads();
	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int d = gg_cdbhash_segment_int8(key[i], nseg);
		unsigned long long idx = lbase[d] + atomicAdd(&lcnt[d], 1ull);

		oa[idx] = a[i];
		if (b)
			ob[idx] = b[i];
		if (c)
			oc[idx] = c[i];
	}
}

hipError_t
launch_part_scatter3(hipStream_t s, const int64_t *key, int64_t n, int nseg,
		     const int64_t *a, const int64_t *b, const int64_t *c,
		     unsigned long long *offsets, int64_t *oa, int64_t *ob,
		     int64_t *oc)
{
	if (nseg > 64)
		return hipErrorInvalidValue;	/* LDS cursor array bound */
	hipLaunchKernelGGL(k_part_scatter3, dim3(grid_for(n)), dim3(THREADS),
			   0, s, key, n, nseg, a, b, c, offsets, oa, ob, oc);
	return hipGetLastError();
}

/* ------------------------------------------------------------------ */
/* Q3 multi-GPU exchange helpers (Motion redistribute legs, §8(e))     */
/* ------------------------------------------------------------------ */

/* orders shard: filter date → compact (ckey, okey, date|prio) triplets */
__global__ void
k_orders_filter_compact(const int64_t *__restrict__ okey,
			const int64_t *__restrict__ ckey,
			const int32_t *__restrict__ odate,
			const int32_t *__restrict__ prio, int64_t n,
			int32_t date_lo, int32_t date_hi,
			int64_t *__restrict__ out_ckey,
			int64_t *__restrict__ out_okey,
			int64_t *__restrict__ out_pay,
			unsigned long long *out_count)
{
	__shared__ unsigned long long lds4[4];
	__shared__ unsigned long long bbase, bcur;
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long my = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int32_t d = nt_ld32(&odate[i]);

		my += (d >= date_lo && d < date_hi);
	}
	block_claim(lds4, &bbase, my, out_count);
	if (threadIdx.x == 0)
		bcur = 0;
	__syncthreads();
	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int32_t d = nt_ld32(&odate[i]);
		bool take = (d >= date_lo && d < date_hi);
		unsigned long long idx = bbase + wave_append(&bcur, take);

		if (!take)
			continue;
		out_ckey[idx] = ckey[i];
		out_okey[idx] = okey[i];
		out_pay[idx] = (int64_t)
			((unsigned long long) (uint32_t) d |
			 ((unsigned long long) (uint32_t) prio[i] << 32));
	}
}

hipError_t
launch_orders_filter_compact(hipStream_t s, const int64_t *okey,
			     const int64_t *ckey, const int32_t *odate,
			     const int32_t *prio, int64_t n, int32_t date_lo,
			     int32_t date_hi, int64_t *out_ckey,
			     int64_t *out_okey, int64_t *out_pay,
			     unsigned long long *out_count)
{
	hipLaunchKernelGGL(k_orders_filter_compact, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, okey, ckey, odate, prio, n,
			   date_lo, date_hi, out_ckey, out_okey, out_pay,
			   out_count);
	return hipGetLastError();
}

/* received (ckey, okey, pay) rows: probe local customer set → compact
 * matched (okey, pay) */
__global__ void
k_probe_cust_compact(const int64_t *__restrict__ ckey,
		     const int64_t *__restrict__ okey,
		     const int64_t *__restrict__ pay, int64_t n,
		     const unsigned long long *__restrict__ cust_keys,
		     uint64_t cust_slots,
		     const unsigned long long *__restrict__ cust_bloom,
		     uint64_t cust_bwords,
		     const unsigned long long *__restrict__ cust_bits,
		     int64_t cust_dlen, int64_t *__restrict__ out_okey,
		     int64_t *__restrict__ out_pay,
		     unsigned long long *out_count)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	__shared__ unsigned long long lds4[4];
	__shared__ unsigned long long bbase, bcur;
	unsigned long long my = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t ck = ckey[i];

		my += cust_bits
			? (ck >= 0 && ck < cust_dlen &&
			   ((cust_bits[ck >> 6] >> (ck & 63)) & 1))
			: ht_contains_b(cust_keys, cust_slots, cust_bloom,
					cust_bwords, ck);
	}
	block_claim(lds4, &bbase, my, out_count);
	if (threadIdx.x == 0)
		bcur = 0;
	__syncthreads();
	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t ck = ckey[i];
		bool take = cust_bits
			? (ck >= 0 && ck < cust_dlen &&
			   ((cust_bits[ck >> 6] >> (ck & 63)) & 1))
			: ht_contains_b(cust_keys, cust_slots, cust_bloom,
					cust_bwords, ck);
		unsigned long long idx = bbase + wave_append(&bcur, take);

		if (!take)
			continue;
		out_okey[idx] = okey[i];
		out_pay[idx] = pay[i];
	}
}

hipError_t
launch_probe_cust_compact(hipStream_t s, const int64_t *ckey,
			  const int64_t *okey, const int64_t *pay, int64_t n,
			  DeviceHashTable cust,
			  const unsigned long long *cust_bits,
			  int64_t cust_dlen, int64_t *out_okey,
			  int64_t *out_pay, unsigned long long *out_count)
{
	hipLaunchKernelGGL(k_probe_cust_compact, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, ckey, okey, pay, n, cust.keys,
			   cust.nslots, cust.bloom, cust.bloom_words,
			   cust_bits, cust_dlen,
			   out_okey, out_pay, out_count);
	return hipGetLastError();
}

/* insert (okey, pay) rows into the orders table */
__global__ void
k_insert_orders(const int64_t *__restrict__ okey,
		const int64_t *__restrict__ pay, int64_t n,
		unsigned long long *__restrict__ tkeys,
		unsigned long long *__restrict__ tpayload, uint64_t nslots,
		unsigned long long *__restrict__ bloom, uint64_t bwords)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t k = okey[i];
		uint64_t pos = ht_start(k, nslots);

		if (bloom)
			bloom_insert(bloom, bwords, k);
		for (;;)
		{
			unsigned long long prev =
				atomicCAS(&tkeys[pos], 0ull,
					  (unsigned long long) k);
			if (prev == 0)
			{
				tpayload[pos] = (unsigned long long) pay[i];
				break;
			}
			if (prev == (unsigned long long) k)
				break;
			pos = (pos + 1) & (nslots - 1);
		}
	}
}

hipError_t
launch_insert_orders(hipStream_t s, const int64_t *okey, const int64_t *pay,
		     int64_t n, DeviceHashTable ord)
{
	hipLaunchKernelGGL(k_insert_orders, dim3(grid_for(n)), dim3(THREADS),
			   0, s, okey, pay, n, ord.keys, ord.payload,
			   ord.nslots, ord.bloom, ord.bloom_words);
	return hipGetLastError();
}


/* ------------------------------------------------------------------ */
/* Q5 (mpph5): supplier/customer dims, orders map, 25-nation agg       */
/* ------------------------------------------------------------------ */

/* generic key→value build: insert every (key, val) pair (the customer
 * c_custkey → c_nationkey map; no filter, so no bloom) */
__global__ void
k_build_kv(const int64_t *__restrict__ keys, const uint8_t *__restrict__ vals,
	   int64_t n, unsigned long long *__restrict__ tkeys,
	   unsigned long long *__restrict__ tpayload, uint64_t nslots)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t k = keys[i];
		uint64_t pos = ht_start(k, nslots);

		for (;;)
		{
			unsigned long long prev =
				atomicCAS(&tkeys[pos], 0ull,
					  (unsigned long long) k);
			if (prev == 0)
			{
				tpayload[pos] = vals[i];
				break;
			}
			if (prev == (unsigned long long) k)
				break;
			pos = (pos + 1) & (nslots - 1);
		}
	}
}

hipError_t
launch_build_kv(hipStream_t s, const int64_t *keys, const uint8_t *vals,
		int64_t n, DeviceHashTable t)
{
	hipLaunchKernelGGL(k_build_kv, dim3(grid_for(n)), dim3(THREADS), 0, s,
			   keys, vals, n, t.keys, t.payload, t.nslots);
	return hipGetLastError();
}

/* probe a kv map; return payload or miss */
__device__ inline bool
ht_lookup_b(const unsigned long long *__restrict__ tkeys,
	    const unsigned long long *__restrict__ tpayload, uint64_t nslots,
	    const unsigned long long *__restrict__ bloom, uint64_t bwords,
	    int64_t key, unsigned long long *out_payload)
{
	uint32_t h = gg_hashint8(key);

	if (bloom && !bloom_maybe(bloom, bwords, h))
		return false;
	{
		uint64_t pos = (uint64_t) h & (nslots - 1);

		for (;;)
		{
			unsigned long long v = tkeys[pos];

			if (v == (unsigned long long) key)
			{
				*out_payload = tpayload[pos];
				return true;
			}
			if (v == 0)
				return false;
			pos = (pos + 1) & (nslots - 1);
		}
	}
}

/* supplier build: keep s_suppkey → s_nationkey for suppliers whose
 * nation is in the target region (the nation⋈region semi-filter pushed
 * into the build, cdbpath-style) */
__global__ void
k_build_supp(const int64_t *__restrict__ suppkey,
	     const uint8_t *__restrict__ snation, int64_t n,
	     const uint8_t *__restrict__ region_of /* [25] device */,
	     uint8_t regionkey, unsigned long long *__restrict__ tkeys,
	     unsigned long long *__restrict__ tpayload, uint64_t nslots,
	     unsigned long long *__restrict__ bloom, uint64_t bwords,
	     unsigned long long *out_count)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long kept = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		uint8_t sn = snation[i];

		if (sn >= 25 || region_of[sn] != regionkey)
			continue;
		kept++;
		{
			int64_t k = suppkey[i];
			uint64_t pos = ht_start(k, nslots);

			if (bloom)
				bloom_insert(bloom, bwords, k);
			for (;;)
			{
				unsigned long long prev =
					atomicCAS(&tkeys[pos], 0ull,
						  (unsigned long long) k);
				if (prev == 0)
				{
					tpayload[pos] = sn;
					break;
				}
				if (prev == (unsigned long long) k)
					break;
				pos = (pos + 1) & (nslots - 1);
			}
		}
	}
	for (int off = 32; off; off >>= 1)
		kept += __shfl_down(kept, off, 64);
	if ((threadIdx.x & 63) == 0 && kept)
		atomicAdd(out_count, kept);
}

hipError_t
launch_build_supp(hipStream_t s, const int64_t *suppkey,
		  const uint8_t *snation, int64_t n, const uint8_t *region_of,
		  uint8_t regionkey, DeviceHashTable t,
		  unsigned long long *out_count)
{
	hipLaunchKernelGGL(k_build_supp, dim3(grid_for(n)), dim3(THREADS), 0,
			   s, suppkey, snation, n, region_of, regionkey,
			   t.keys, t.payload, t.nslots, t.bloom,
			   t.bloom_words, out_count);
	return hipGetLastError();
}

/* supplier shard → compacted (suppkey, nation) pairs for the broadcast
 * Motion (in-region only) */
__global__ void
k_supp_filter_compact(const int64_t *__restrict__ suppkey,
		      const uint8_t *__restrict__ snation, int64_t n,
		      const uint8_t *__restrict__ region_of, uint8_t regionkey,
		      int64_t *__restrict__ out_sk,
		      int64_t *__restrict__ out_sn,
		      unsigned long long *out_count)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	__shared__ unsigned long long lds4[4];
	__shared__ unsigned long long bbase, bcur;
	unsigned long long my = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		uint8_t sn = snation[i];

		my += (sn < 25 && region_of[sn] == regionkey);
	}
	block_claim(lds4, &bbase, my, out_count);
	if (threadIdx.x == 0)
		bcur = 0;
	__syncthreads();
	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		uint8_t sn = snation[i];
		bool take = (sn < 25 && region_of[sn] == regionkey);
		unsigned long long idx = bbase + wave_append(&bcur, take);

		if (!take)
			continue;
		out_sk[idx] = suppkey[i];
		out_sn[idx] = sn;
	}
}

hipError_t
launch_supp_filter_compact(hipStream_t s, const int64_t *suppkey,
			   const uint8_t *snation, int64_t n,
			   const uint8_t *region_of, uint8_t regionkey,
			   int64_t *out_sk, int64_t *out_sn,
			   unsigned long long *out_count)
{
	hipLaunchKernelGGL(k_supp_filter_compact, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, suppkey, snation, n,
			   region_of, regionkey, out_sk, out_sn, out_count);
	return hipGetLastError();
}

/* insert broadcast (suppkey, nation-as-i64) pairs into the supp table */
__global__ void
k_insert_supp(const int64_t *__restrict__ sk, const int64_t *__restrict__ sn,
	      int64_t n, unsigned long long *__restrict__ tkeys,
	      unsigned long long *__restrict__ tpayload, uint64_t nslots,
	      unsigned long long *__restrict__ bloom, uint64_t bwords)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t k = sk[i];
		uint64_t pos = ht_start(k, nslots);

		if (bloom)
			bloom_insert(bloom, bwords, k);
		for (;;)
		{
			unsigned long long prev =
				atomicCAS(&tkeys[pos], 0ull,
					  (unsigned long long) k);
			if (prev == 0)
			{
				tpayload[pos] = (unsigned long long) sn[i];
				break;
			}
			if (prev == (unsigned long long) k)
				break;
			pos = (pos + 1) & (nslots - 1);
		}
	}
}

hipError_t
launch_insert_supp(hipStream_t s, const int64_t *sk, const int64_t *sn,
		   int64_t n, DeviceHashTable t)
{
	hipLaunchKernelGGL(k_insert_supp, dim3(grid_for(n)), dim3(THREADS),
			   0, s, sk, sn, n, t.keys, t.payload, t.nslots,
			   t.bloom, t.bloom_words);
	return hipGetLastError();
}

/* orders (fused, single-segment): date range filter, probe customer
 * map, insert okey → c_nationkey */
__global__ void
k_build_orders_q5(const int64_t *__restrict__ okey,
		  const int64_t *__restrict__ ckey,
		  const int32_t *__restrict__ odate, int64_t n,
		  int32_t date_lo, int32_t date_hi,
		  const unsigned long long *__restrict__ cust_keys,
		  const unsigned long long *__restrict__ cust_pay,
		  uint64_t cust_slots,
		  const uint8_t *__restrict__ cust_dense, int64_t cust_dlen,
		  unsigned long long *__restrict__ tkeys,
		  unsigned long long *__restrict__ tpayload, uint64_t nslots,
		  unsigned long long *__restrict__ bloom, uint64_t bwords,
		  unsigned long long *match_count)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long matches = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int32_t d = odate[i];
		unsigned long long nat;

		if (d < date_lo || d >= date_hi)
			continue;
		if (cust_dense)
		{
			int64_t ck = ckey[i];

			if (ck < 0 || ck >= cust_dlen || cust_dense[ck] == 255)
				continue;
			nat = cust_dense[ck];
		}
		else if (!ht_lookup_b(cust_keys, cust_pay, cust_slots, nullptr,
				      0, ckey[i], &nat))
			continue;	/* inner join: unmatched drops */
		matches++;
		{
			int64_t k = okey[i];
			uint64_t pos = ht_start(k, nslots);

			if (bloom)
				bloom_insert(bloom, bwords, k);
			for (;;)
			{
				unsigned long long prev =
					atomicCAS(&tkeys[pos], 0ull,
						  (unsigned long long) k);
				if (prev == 0)
				{
					tpayload[pos] = nat;
					break;
				}
				if (prev == (unsigned long long) k)
					break;
				pos = (pos + 1) & (nslots - 1);
			}
		}
	}
	for (int off = 32; off; off >>= 1)
		matches += __shfl_down(matches, off, 64);
	if ((threadIdx.x & 63) == 0 && matches)
		atomicAdd(match_count, matches);
}

hipError_t
launch_build_orders_q5(hipStream_t s, const int64_t *okey,
		       const int64_t *ckey, const int32_t *odate, int64_t n,
		       int32_t date_lo, int32_t date_hi, DeviceHashTable cust,
		       const uint8_t *cust_dense, int64_t cust_dlen,
		       DeviceHashTable ord, unsigned long long *match_count)
{
	hipLaunchKernelGGL(k_build_orders_q5, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, okey, ckey, odate, n,
			   date_lo, date_hi, cust.keys, cust.payload,
			   cust.nslots, cust_dense, cust_dlen,
			   ord.keys, ord.payload, ord.nslots,
			   ord.bloom, ord.bloom_words, match_count);
	return hipGetLastError();
}

/* count orders in [lo, hi) — exact-sizing pass */
__global__ void
k_count_date_range(const int32_t *__restrict__ odate, int64_t n,
		   int32_t date_lo, int32_t date_hi,
		   unsigned long long *out)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long c = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
		c += (odate[i] >= date_lo && odate[i] < date_hi);
	for (int off = 32; off; off >>= 1)
		c += __shfl_down(c, off, 64);
	if ((threadIdx.x & 63) == 0 && c)
		atomicAdd(out, c);
}

hipError_t
launch_count_date_range(hipStream_t s, const int32_t *odate, int64_t n,
			int32_t date_lo, int32_t date_hi,
			unsigned long long *out)
{
	hipLaunchKernelGGL(k_count_date_range, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, odate, n, date_lo, date_hi,
			   out);
	return hipGetLastError();
}

/* received (ckey, okey) rows: probe customer MAP → (okey, nation) */
__global__ void
k_probe_cust_map_compact(const int64_t *__restrict__ ckey,
			 const int64_t *__restrict__ okey, int64_t n,
			 const unsigned long long *__restrict__ cust_keys,
			 const unsigned long long *__restrict__ cust_pay,
			 uint64_t cust_slots,
			 const uint8_t *__restrict__ cust_dense,
			 int64_t cust_dlen, int64_t *__restrict__ out_okey,
			 int64_t *__restrict__ out_nat,
			 unsigned long long *out_count)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	__shared__ unsigned long long lds4[4];
	__shared__ unsigned long long bbase, bcur;
	unsigned long long my = 0;

	auto look = [&](int64_t i, unsigned long long *nat) -> bool
	{
		if (cust_dense)
		{
			int64_t ck = ckey[i];
			bool t = (ck >= 0 && ck < cust_dlen &&
				  cust_dense[ck] != 255);

			if (t)
				*nat = cust_dense[ck];
			return t;
		}
		return ht_lookup_b(cust_keys, cust_pay, cust_slots, nullptr,
				   0, ckey[i], nat);
	};

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		unsigned long long nat = 0;

		my += look(i, &nat);
	}
	block_claim(lds4, &bbase, my, out_count);
	if (threadIdx.x == 0)
		bcur = 0;
	__syncthreads();
	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		unsigned long long nat = 0;
		bool take = look(i, &nat);
		unsigned long long idx = bbase + wave_append(&bcur, take);

		if (!take)
			continue;
		out_okey[idx] = okey[i];
		out_nat[idx] = (int64_t) nat;
	}
}

hipError_t
launch_probe_cust_map_compact(hipStream_t s, const int64_t *ckey,
			      const int64_t *okey, int64_t n,
			      DeviceHashTable cust, const uint8_t *cust_dense,
			      int64_t cust_dlen, int64_t *out_okey,
			      int64_t *out_nat, unsigned long long *out_count)
{
	hipLaunchKernelGGL(k_probe_cust_map_compact, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, ckey, okey, n, cust.keys,
			   cust.payload, cust.nslots, cust_dense, cust_dlen,
			   out_okey, out_nat, out_count);
	return hipGetLastError();
}

/* lineitem probe: supplier (small, bloom) then orders (bloom), nation
 * equality, 25-slot LDS-privatized aggregation.
 * acc layout: [nation][0]=count, [nation][1]=rev_lo, [nation][2]=rev_hi */
__global__ __launch_bounds__(THREADS, 2)
void k_probe_lineitem_q5(const int64_t *__restrict__ okey,
			 const int64_t *__restrict__ skey,
			 const int64_t *__restrict__ price,
			 const int64_t *__restrict__ disc, int64_t n,
			 const unsigned long long *__restrict__ ord_keys,
			 const unsigned long long *__restrict__ ord_pay,
			 uint64_t ord_slots,
			 const unsigned long long *__restrict__ ord_bloom,
			 uint64_t ord_bwords,
			 const unsigned long long *__restrict__ supp_keys,
			 const unsigned long long *__restrict__ supp_pay,
			 uint64_t supp_slots,
			 const unsigned long long *__restrict__ supp_bloom,
			 uint64_t supp_bwords,
			 const uint8_t *__restrict__ supp_dense,
			 int64_t supp_dense_len,
			 unsigned long long *__restrict__ acc /* [25][3] */,
			 unsigned long long *join_rows)
{
	__shared__ unsigned long long lds[25][2];	/* cnt, rev */

	for (int i = threadIdx.x; i < 50; i += blockDim.x)
		((unsigned long long *) lds)[i] = 0;
	__syncthreads();

	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long joined = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		/* both keys loaded densely (coalesced), both Bloom filters
		 * tested before any slot-array probe: sparse exec-masked
		 * loads mid-kernel cost a full cache line per surviving
		 * lane, so the cheap rejections come first */
		int64_t sk = nt_ld64(&skey[i]);
		int64_t ok = nt_ld64(&okey[i]);
		unsigned long long snat, onat;

		if (supp_dense)
		{
			/* dense path: one L2-resident byte lookup */
			if (sk < 0 || sk >= supp_dense_len)
				continue;
			snat = supp_dense[sk];
			if (snat == 255)
				continue;
		}
		else
		{
			uint32_t hsk = gg_hashint8(sk);

			if (supp_bloom &&
			    !bloom_maybe(supp_bloom, supp_bwords, hsk))
				continue;
			if (!ht_lookup_b(supp_keys, supp_pay, supp_slots,
					 nullptr, 0, sk, &snat))
				continue;
		}
		{
			uint32_t hok = gg_hashint8(ok);

			if (ord_bloom &&
			    !bloom_maybe(ord_bloom, ord_bwords, hok))
				continue;
			if (!ht_lookup_b(ord_keys, ord_pay, ord_slots,
					 nullptr, 0, ok, &onat))
				continue;
		}
		if (snat != onat)	/* c_nationkey = s_nationkey */
			continue;
		joined++;
		{
			unsigned long long rev4 = (unsigned long long)
				(price[i] * (100 - disc[i]));

			atomicAdd(&lds[snat][0], 1ull);
			atomicAdd(&lds[snat][1], rev4);
		}
	}
	for (int off = 32; off; off >>= 1)
		joined += __shfl_down(joined, off, 64);
	if ((threadIdx.x & 63) == 0 && joined)
		atomicAdd(join_rows, joined);
	__syncthreads();
	for (int nat = threadIdx.x; nat < 25; nat += blockDim.x)
	{
		unsigned long long c = lds[nat][0];
		unsigned long long r = lds[nat][1];

		if (!c)
			continue;
		atomicAdd(&acc[nat * 3 + 0], c);
		{
			unsigned long long old =
				atomicAdd(&acc[nat * 3 + 1], r);
			if (old + r < old)
				atomicAdd(&acc[nat * 3 + 2], 1ull);
		}
	}
}

hipError_t
launch_probe_lineitem_q5(hipStream_t s, const int64_t *okey,
			 const int64_t *skey, const int64_t *price,
			 const int64_t *disc, int64_t n, DeviceHashTable ord,
			 DeviceHashTable supp, const uint8_t *supp_dense,
			 int64_t supp_dense_len, unsigned long long *acc,
			 unsigned long long *join_rows)
{
	hipLaunchKernelGGL(k_probe_lineitem_q5, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, okey, skey, price, disc, n,
			   ord.keys, ord.payload, ord.nslots, ord.bloom,
			   ord.bloom_words, supp.keys, supp.payload,
			   supp.nslots, supp.bloom, supp.bloom_words,
			   supp_dense, supp_dense_len, acc, join_rows);
	return hipGetLastError();
}

__global__ void
k_gen_supplier(uint64_t seed, int64_t row_lo, int64_t n, int nseg, int seg,
	       int64_t *__restrict__ suppkey, uint8_t *__restrict__ nation,
	       unsigned long long *out_count)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t sk = row_lo + i + 1;
		bool own = (nseg <= 1) ||
			(gg_cdbhash_segment_int8(sk, nseg) == seg);
		int64_t idx = i;

		if (nseg > 1)
		{
			unsigned long long mask = __ballot(own);
			int lane = threadIdx.x & 63;
			int nbefore = __popcll(mask & ((1ull << lane) - 1));
			int total = __popcll(mask);
			int leader = __ffsll((long long) mask) - 1;
			unsigned long long base = 0;

			if (total && lane == leader)
				base = atomicAdd(out_count,
						 (unsigned long long) total);
			if (total)
				base = __shfl(base, leader, 64);
			idx = (int64_t) (base + (unsigned) nbefore);
		}
		if (!own)
			continue;
		suppkey[idx] = sk;
		nation[idx] = gg_s_nationkey(seed, sk);
	}
}

hipError_t
launch_gen_supplier(hipStream_t s, uint64_t seed, int64_t row_lo, int64_t n,
		    int nseg, int seg, int64_t *suppkey, uint8_t *nation,
		    unsigned long long *out_count)
{
	hipLaunchKernelGGL(k_gen_supplier, dim3(grid_for(n)), dim3(THREADS),
			   0, s, seed, row_lo, n, nseg, seg, suppkey, nation,
			   out_count);
	return hipGetLastError();
}


/* ------------------------------------------------------------------ */
/* general hash group-by: arbitrary int64 keys, many groups            */
/* (execHHashagg.c:456 lookup_agg_hash_entry semantics: find-or-create */
/* group, transition per row; open addressing, EMPTY = INT64_MIN)      */
/* ------------------------------------------------------------------ */

#define GB_EMPTY 0x8000000000000000ull	/* INT64_MIN as the empty slot */

/* narrow decoded int32 values into a u8 column (char1/dict codes) */
__global__ void
k_narrow_i32_u8(const int32_t *__restrict__ in, int64_t n,
		uint8_t *__restrict__ out)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
		out[i] = (uint8_t) in[i];
}

hipError_t
launch_narrow_i32_u8(hipStream_t s, const int32_t *in, int64_t n,
		     uint8_t *out)
{
	hipLaunchKernelGGL(k_narrow_i32_u8, dim3(grid_for(n)), dim3(THREADS),
			   0, s, in, n, out);
	return hipGetLastError();
}

/* generic i64-key hash-join kernels for the spill tier
 * (ExecHashJoin batching semantics, nodeHash.c:713): CAS-insert build
 * (key 0 reserved as empty, like the pipeline tables), probe emits
 * (probe_row_index, build_val) matches via wave-aggregated append.
 * The build refuses what the table cannot represent: a key 0 (it would
 * "match" the first empty slot without occupying it) raises
 * SJ_ERR_ZERO_KEY in *err, a key already in the table (the CAS hands the
 * key itself back to exactly one of the two rows) SJ_ERR_DUP_KEY; the
 * host turns either into GG_EINVAL.  A probe key 0 matches nothing. */
__global__ void
k_sj_build(const int64_t *__restrict__ keys,
	   const int64_t *__restrict__ vals, int64_t n,
	   unsigned long long *__restrict__ tkeys,
	   unsigned long long *__restrict__ tvals, uint64_t nslots,
	   unsigned long long *__restrict__ err)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t kk = keys[i];
		uint64_t pos = (uint64_t) gg_hashint8(kk) & (nslots - 1);

		if (kk == 0)
		{
			atomicOr(err, SJ_ERR_ZERO_KEY);
			continue;
		}
		for (;;)
		{
			unsigned long long prev =
				atomicCAS(&tkeys[pos], 0ull,
					  (unsigned long long) kk);

			if (prev == 0)
			{
				tvals[pos] = (unsigned long long) vals[i];
				break;
			}
			if (prev == (unsigned long long) kk)
			{
				atomicOr(err, SJ_ERR_DUP_KEY);
				break;
			}
			pos = (pos + 1) & (nslots - 1);
		}
	}
}

__global__ void
k_sj_probe(const int64_t *__restrict__ keys,
	   const int64_t *__restrict__ idxs, int64_t n,
	   const unsigned long long *__restrict__ tkeys,
	   const unsigned long long *__restrict__ tvals, uint64_t nslots,
	   int64_t *__restrict__ out_idx, int64_t *__restrict__ out_val,
	   unsigned long long *out_count)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	const int64_t i0 = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	__shared__ unsigned long long lds4[4];
	__shared__ unsigned long long bbase, bcur;
	unsigned long long my = 0;

	auto probe = [&](int64_t i, unsigned long long *v) -> bool
	{
		int64_t kk = keys[i];
		uint64_t pos = (uint64_t) gg_hashint8(kk) & (nslots - 1);

		if (kk == 0)	/* would equal the first empty slot */
			return false;
		for (;;)
		{
			unsigned long long cur = tkeys[pos];

			if (cur == (unsigned long long) kk)
			{
				*v = tvals[pos];
				return true;
			}
			if (cur == 0)
				return false;
			pos = (pos + 1) & (nslots - 1);
		}
	};

	/* block-claimed append (the per-wave global counter serializes
	 * at the ~88 atomics/µs wall): count, claim once, write */
	for (int64_t i = i0; i < n; i += stride)
	{
		unsigned long long v;

		my += probe(i, &v);
	}
	block_claim(lds4, &bbase, my, out_count);
	if (threadIdx.x == 0)
		bcur = 0;
	__syncthreads();
	{
		const int64_t n_up = ((n + stride - 1) / stride) * stride;

		for (int64_t i = i0; i < n_up; i += stride)
		{
			bool hit = false;
			unsigned long long v = 0;

			if (i < n)
				hit = probe(i, &v);
			{
				unsigned long long at = bbase +
					wave_append(&bcur, hit);

				if (hit)
				{
					out_idx[at] = idxs[i];
					out_val[at] = (int64_t) v;
				}
			}
		}
	}
}

hipError_t
launch_sj_build(hipStream_t s, const int64_t *keys, const int64_t *vals,
		int64_t n, unsigned long long *tkeys,
		unsigned long long *tvals, uint64_t nslots,
		unsigned long long *err)
{
	hipLaunchKernelGGL(k_sj_build, dim3(grid_for(n)), dim3(THREADS), 0,
			   s, keys, vals, n, tkeys, tvals, nslots, err);
	return hipGetLastError();
}

hipError_t
launch_sj_probe(hipStream_t s, const int64_t *keys, const int64_t *idxs,
		int64_t n, const unsigned long long *tkeys,
		const unsigned long long *tvals, uint64_t nslots,
		int64_t *out_idx, int64_t *out_val,
		unsigned long long *out_count)
{
	hipLaunchKernelGGL(k_sj_probe, dim3(grid_for(n)), dim3(THREADS), 0,
			   s, keys, idxs, n, tkeys, tvals, nslots, out_idx,
			   out_val, out_count);
	return hipGetLastError();
}

/* variant of the partition scatter that carries the ORIGINAL row index
 * (base + i) as the value — used to keep probe-row identity through
 * the spill partitioning without materializing an iota on the host */
__global__ void
k_gb_part_scatter_idx(const int64_t *__restrict__ keys, int64_t n,
		      int64_t base, int shift,
		      unsigned long long *__restrict__ cursors,
		      int64_t *__restrict__ out_k,
		      int64_t *__restrict__ out_v)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		uint64_t p = (uint64_t) gg_hashint8(keys[i]) >> shift;
		unsigned long long at = atomicAdd(&cursors[p], 1ull);

		out_k[at] = keys[i];
		out_v[at] = base + i;
	}
}


/* hash-range partitioning for the spill tier (execHHashagg.c:1350
 * spill_hash_table semantics): partition id = TOP bits of the key
 * hash, decoupled from the group table's slot index (low bits) */
/* spill-tier partitions are <= 4096 but almost always <= 1024:
 * the LDS-staged form covers that; the launchers fall back to the
 * direct-atomic form above it (suffix _direct) otherwise */
#define GB_LDS_PARTS 1024

template <int LDS>
__global__ void
k_gb_part_count_t(const int64_t *__restrict__ keys, int64_t n, int shift,
		  unsigned long long *__restrict__ counts)
{
	__shared__ unsigned long long lcnt[LDS ? GB_LDS_PARTS : 1];
	const int nparts = (int) ((uint64_t) 0xffffffffu >> shift) + 1;

	if (LDS)
	{
		for (int d = threadIdx.x; d < nparts; d += blockDim.x)
			lcnt[d] = 0;
		__syncthreads();
	}

	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		/* 64-bit shift: shift==32 (single partition) must yield 0 */
		uint64_t p = (uint64_t) gg_hashint8(keys[i]) >> shift;

		if (LDS)
			atomicAdd(&lcnt[p], 1ull);
		else
			atomicAdd(&counts[p], 1ull);
	}
	if (LDS)
	{
		__syncthreads();
		for (int d = threadIdx.x; d < nparts; d += blockDim.x)
			if (lcnt[d])
				atomicAdd(&counts[d], lcnt[d]);
	}
}

/* block-claimed scatter: count per block in LDS, claim one region per
 * (block, partition), append through LDS cursors (VAL==1: payload =
 * vals[i]; VAL==0: payload = base + i, the index-carrying variant) */
template <int VAL>
__global__ void
k_gb_part_scatter_t(const int64_t *__restrict__ keys,
		    const int64_t *__restrict__ vals, int64_t n,
		    int64_t base, int shift,
		    unsigned long long *__restrict__ cursors,
		    int64_t *__restrict__ out_k, int64_t *__restrict__ out_v)
{
	__shared__ unsigned long long lcnt[GB_LDS_PARTS];
	__shared__ unsigned long long lbase[GB_LDS_PARTS];
	const int nparts = (int) ((uint64_t) 0xffffffffu >> shift) + 1;
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int d = threadIdx.x; d < nparts; d += blockDim.x)
		lcnt[d] = 0;
	__syncthreads();
	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
		atomicAdd(&lcnt[(uint64_t) gg_hashint8(keys[i]) >> shift],
			  1ull);
	__syncthreads();
	for (int d = threadIdx.x; d < nparts; d += blockDim.x)
	{
		lbase[d] = lcnt[d] ? atomicAdd(&cursors[d], lcnt[d]) : 0;
		lcnt[d] = 0;
	}
	__syncthreads();
	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		uint64_t p = (uint64_t) gg_hashint8(keys[i]) >> shift;
		unsigned long long at = lbase[p] + atomicAdd(&lcnt[p], 1ull);

		out_k[at] = keys[i];
		out_v[at] = VAL ? vals[i] : base + i;
	}
}

__global__ void
k_gb_part_scatter(const int64_t *__restrict__ keys,
		  const int64_t *__restrict__ vals, int64_t n, int shift,
		  unsigned long long *__restrict__ cursors,
		  int64_t *__restrict__ out_k, int64_t *__restrict__ out_v)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		uint64_t p = (uint64_t) gg_hashint8(keys[i]) >> shift;
		unsigned long long at = atomicAdd(&cursors[p], 1ull);

		out_k[at] = keys[i];
		out_v[at] = vals[i];
	}
}

/* tiny on-device exclusive prefix over the partition counts: writes a
 * WORKING cursor copy (consumed by the scatter's atomics) and a
 * PRISTINE copy (+ total) for the host's staging distribution — keeps
 * the spill partition pipeline free of mid-chunk host syncs.  P <=
 * 4096: one thread's serial scan is ~us and fully overlapped. */
__global__ void
k_gb_prefix2_u64(const unsigned long long *__restrict__ cnt, int n,
		 unsigned long long *__restrict__ work,
		 unsigned long long *__restrict__ pristine)
{
	if (blockIdx.x == 0 && threadIdx.x == 0)
	{
		unsigned long long s = 0;

		for (int i = 0; i < n; i++)
		{
			work[i] = s;
			pristine[i] = s;
			s += cnt[i];
		}
		pristine[n] = s;
	}
}

hipError_t
launch_gb_prefix2_u64(hipStream_t s, const unsigned long long *cnt, int n,
		      unsigned long long *work, unsigned long long *pristine)
{
	hipLaunchKernelGGL(k_gb_prefix2_u64, dim3(1), dim3(64), 0, s,
			   cnt, n, work, pristine);
	return hipGetLastError();
}

static inline int gb_nparts(int shift)
{
	return (int) ((uint64_t) 0xffffffffu >> shift) + 1;
}

hipError_t
launch_gb_part_scatter_idx(hipStream_t s, const int64_t *keys, int64_t n,
			   int64_t base, int shift,
			   unsigned long long *cursors, int64_t *out_k,
			   int64_t *out_v)
{
	if (gb_nparts(shift) <= GB_LDS_PARTS)
		hipLaunchKernelGGL((k_gb_part_scatter_t<0>),
				   dim3(grid_for(n)), dim3(THREADS), 0, s,
				   keys, nullptr, n, base, shift, cursors,
				   out_k, out_v);
	else
		hipLaunchKernelGGL(k_gb_part_scatter_idx, dim3(grid_for(n)),
				   dim3(THREADS), 0, s, keys, n, base, shift,
				   cursors, out_k, out_v);
	return hipGetLastError();
}


hipError_t
launch_gb_part_count(hipStream_t s, const int64_t *keys, int64_t n,
		     int shift, unsigned long long *counts)
{
	if (gb_nparts(shift) <= GB_LDS_PARTS)
		hipLaunchKernelGGL((k_gb_part_count_t<1>), dim3(grid_for(n)),
				   dim3(THREADS), 0, s, keys, n, shift,
				   counts);
	else
		hipLaunchKernelGGL((k_gb_part_count_t<0>), dim3(grid_for(n)),
				   dim3(THREADS), 0, s, keys, n, shift,
				   counts);
	return hipGetLastError();
}

hipError_t
launch_gb_part_scatter(hipStream_t s, const int64_t *keys,
		       const int64_t *vals, int64_t n, int shift,
		       unsigned long long *cursors, int64_t *out_k,
		       int64_t *out_v)
{
	if (gb_nparts(shift) <= GB_LDS_PARTS)
		hipLaunchKernelGGL((k_gb_part_scatter_t<1>),
				   dim3(grid_for(n)), dim3(THREADS), 0, s,
				   keys, vals, n, 0, shift, cursors, out_k,
				   out_v);
	else
		hipLaunchKernelGGL(k_gb_part_scatter, dim3(grid_for(n)),
				   dim3(THREADS), 0, s, keys, vals, n, shift,
				   cursors, out_k, out_v);
	return hipGetLastError();
}

__global__ void
k_groupby_build(const int64_t *__restrict__ keys,
		const int64_t *__restrict__ vals, int64_t n,
		unsigned long long *__restrict__ tkeys,
		unsigned long long *__restrict__ tsum,
		unsigned long long *__restrict__ tcnt, uint64_t nslots,
		unsigned long long *__restrict__ err)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t k = nt_ld64(&keys[i]);
		int64_t v = nt_ld64(&vals[i]);
		uint64_t pos = (uint64_t) gg_hashint8(k) & (nslots - 1);

		/* the empty sentinel as a key would add into the first empty
		 * slot without claiming it: refuse the row, the host reports
		 * GG_EINVAL */
		if ((unsigned long long) k == GB_EMPTY)
		{
			atomicOr(err, 1ull);
			continue;
		}
		for (;;)
		{
			unsigned long long cur = tkeys[pos];

			if (cur == (unsigned long long) k)
				break;
			if (cur == GB_EMPTY)
			{
				unsigned long long prev =
					atomicCAS(&tkeys[pos], GB_EMPTY,
						  (unsigned long long) k);
				if (prev == GB_EMPTY ||
				    prev == (unsigned long long) k)
					break;
			}
			pos = (pos + 1) & (nslots - 1);
		}
		/* wrapping u64 add == two's-complement int64 sum */
		atomicAdd(&tsum[pos], (unsigned long long) v);
		atomicAdd(&tcnt[pos], 1ull);
	}
}

__global__ void
k_groupby_compact(const unsigned long long *__restrict__ tkeys,
		  const unsigned long long *__restrict__ tsum,
		  const unsigned long long *__restrict__ tcnt,
		  uint64_t nslots, int64_t *__restrict__ out_keys,
		  int64_t *__restrict__ out_sums,
		  int64_t *__restrict__ out_cnts,
		  unsigned long long *out_n, uint64_t cap)
{
	const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;

	for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < nslots; i += stride)
	{
		bool take = (tkeys[i] != GB_EMPTY);
		unsigned long long idx = wave_append(out_n, take);

		if (!take || idx >= cap)
			continue;
		out_keys[idx] = (int64_t) tkeys[i];
		out_sums[idx] = (int64_t) tsum[i];
		out_cnts[idx] = (int64_t) tcnt[i];
	}
}

hipError_t
launch_groupby_build(hipStream_t s, const int64_t *keys, const int64_t *vals,
		     int64_t n, unsigned long long *tkeys,
		     unsigned long long *tsum, unsigned long long *tcnt,
		     uint64_t nslots, unsigned long long *err)
{
	hipLaunchKernelGGL(k_groupby_build, dim3(grid_for(n)), dim3(THREADS),
			   0, s, keys, vals, n, tkeys, tsum, tcnt, nslots, err);
	return hipGetLastError();
}

hipError_t
launch_groupby_compact(hipStream_t s, const unsigned long long *tkeys,
		       const unsigned long long *tsum,
		       const unsigned long long *tcnt, uint64_t nslots,
		       int64_t *out_keys, int64_t *out_sums,
		       int64_t *out_cnts, unsigned long long *out_n,
		       uint64_t cap)
{
	hipLaunchKernelGGL(k_groupby_compact,
			   dim3(grid_for((int64_t) nslots)), dim3(THREADS),
			   0, s, tkeys, tsum, tcnt, nslots, out_keys,
			   out_sums, out_cnts, out_n, cap);
	return hipGetLastError();
}

__global__ void
k_fill_u64(unsigned long long *__restrict__ p, uint64_t n,
	   unsigned long long v)
{
	const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;

	for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
		p[i] = v;
}

hipError_t
launch_fill_u64(hipStream_t s, unsigned long long *p, uint64_t n,
		unsigned long long v)
{
	hipLaunchKernelGGL(k_fill_u64, dim3(grid_for((int64_t) n)),
			   dim3(THREADS), 0, s, p, n, v);
	return hipGetLastError();
}


/* dense supplier side: when s_suppkey is (near-)dense the whole
 * in-region supplier map collapses to a u8 array (suppkey -> nation,
 * 255 = absent) that lives in L2 — one byte load replaces bloom+table
 * probes.  Guarded by max_key <= 8*nrows at build; hash fallback
 * otherwise. */
__global__ void
k_max_i64(const int64_t *__restrict__ v, int64_t n,
	  unsigned long long *out_max)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long m = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t x = nt_ld64(&v[i]);

		/* a negative key poisons the result to ~0 so every
		 * dense-path sizing guard (unsigned compare against
		 * 8*rows) rejects the column: the dense bitmap/array
		 * builds index by key and would silently drop negative
		 * keys, diverging from the reference's hash join */
		if (x < 0)
			m = ~0ull;
		else if ((unsigned long long) x > m)
			m = (unsigned long long) x;
	}
	for (int off = 32; off; off >>= 1)
	{
		unsigned long long o = __shfl_down(m, off, 64);

		if (o > m)
			m = o;
	}
	if ((threadIdx.x & 63) == 0 && m)
		atomicMax(out_max, m);
}

hipError_t
launch_max_i64(hipStream_t s, const int64_t *v, int64_t n,
	       unsigned long long *out_max)
{
	hipLaunchKernelGGL(k_max_i64, dim3(grid_for(n)), dim3(THREADS), 0, s,
			   v, n, out_max);
	return hipGetLastError();
}

/* signed min/max of a column (width 1/4/8), order-encoded into u64
 * (x ^ sign bit) so LDS-free atomicMin/Max work; host seeds
 * out2 = {~0, 0} and decodes.  Feeds the aggregate overflow-budget
 * proof for the baked plan kernel (plan.cpp). */
template <int W>
__global__ void
k_minmax_i64(const void *__restrict__ vp, int64_t n,
	     unsigned long long *out2)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;
	unsigned long long mn = ~0ull, mx = 0;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t x = W == 1 ? (int64_t) ((const uint8_t *) vp)[i]
			: W == 4 ? (int64_t) ((const int32_t *) vp)[i]
			: ((const int64_t *) vp)[i];
		unsigned long long e = (unsigned long long) x
			^ 0x8000000000000000ull;

		if (e < mn)
			mn = e;
		if (e > mx)
			mx = e;
	}
	for (int off = 32; off; off >>= 1)
	{
		unsigned long long a = __shfl_down(mn, off, 64);
		unsigned long long b = __shfl_down(mx, off, 64);

		if (a < mn)
			mn = a;
		if (b > mx)
			mx = b;
	}
	if ((threadIdx.x & 63) == 0)
	{
		atomicMin(&out2[0], mn);
		atomicMax(&out2[1], mx);
	}
}

hipError_t
launch_minmax_i64(hipStream_t s, const void *v, int width, int64_t n,
		  unsigned long long *out2)
{
	dim3 g(grid_for(n)), b(THREADS);

	if (width == 1)
		hipLaunchKernelGGL(k_minmax_i64<1>, g, b, 0, s, v, n, out2);
	else if (width == 4)
		hipLaunchKernelGGL(k_minmax_i64<4>, g, b, 0, s, v, n, out2);
	else
		hipLaunchKernelGGL(k_minmax_i64<8>, g, b, 0, s, v, n, out2);
	return hipGetLastError();
}

__global__ void
k_supp_dense_fill(const int64_t *__restrict__ suppkey,
		  const uint8_t *__restrict__ snation, int64_t n,
		  const uint8_t *__restrict__ region_of, uint8_t regionkey,
		  uint8_t *__restrict__ dense, int64_t dense_len)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		uint8_t sn = snation[i];
		int64_t k = suppkey[i];

		if (k < 0 || k >= dense_len)
			continue;
		if (sn < 25 && region_of[sn] == regionkey)
			dense[k] = sn;
	}
}

hipError_t
launch_supp_dense_fill(hipStream_t s, const int64_t *suppkey,
		       const uint8_t *snation, int64_t n,
		       const uint8_t *region_of, uint8_t regionkey,
		       uint8_t *dense, int64_t dense_len)
{
	hipLaunchKernelGGL(k_supp_dense_fill, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, suppkey, snation, n,
			   region_of, regionkey, dense, dense_len);
	return hipGetLastError();
}

/* dense fill from broadcast (suppkey, nation-as-i64) pairs */
__global__ void
k_supp_dense_fill_pairs(const int64_t *__restrict__ sk,
			const int64_t *__restrict__ sn, int64_t n,
			uint8_t *__restrict__ dense, int64_t dense_len)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t k = sk[i];

		if (k >= 0 && k < dense_len)
			dense[k] = (uint8_t) sn[i];
	}
}

hipError_t
launch_supp_dense_fill_pairs(hipStream_t s, const int64_t *sk,
			     const int64_t *sn, int64_t n, uint8_t *dense,
			     int64_t dense_len)
{
	hipLaunchKernelGGL(k_supp_dense_fill_pairs, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, sk, sn, n, dense, dense_len);
	return hipGetLastError();
}


/* dense customer side (guarded like the supplier one): when c_custkey
 * is (near-)dense, the customer build side collapses to a u8 array —
 * Q3: 1 = in the mktsegment, 0 = not; Q5: nationkey, 255 = absent.
 * One L2/L3-resident byte load replaces bloom + 512 MB-table probes. */
__global__ void
k_cust_dense_fill_seg(const int64_t *__restrict__ custkey,
		      const uint8_t *__restrict__ mktseg, int64_t n,
		      uint8_t segcode, unsigned long long *__restrict__ bits,
		      int64_t dense_len)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t k = custkey[i];

		if (k >= 0 && k < dense_len && mktseg[i] == segcode)
			atomicOr(&bits[k >> 6], 1ull << (k & 63));
	}
}

hipError_t
launch_cust_dense_fill_seg(hipStream_t s, const int64_t *custkey,
			   const uint8_t *mktseg, int64_t n, uint8_t segcode,
			   unsigned long long *bits, int64_t dense_len)
{
	hipLaunchKernelGGL(k_cust_dense_fill_seg, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, custkey, mktseg, n, segcode,
			   bits, dense_len);
	return hipGetLastError();
}

__global__ void
k_cust_dense_fill_nat(const int64_t *__restrict__ custkey,
		      const uint8_t *__restrict__ nation, int64_t n,
		      uint8_t *__restrict__ dense, int64_t dense_len)
{
	const int64_t stride = (int64_t) gridDim.x * blockDim.x;

	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	     i < n; i += stride)
	{
		int64_t k = custkey[i];

		if (k >= 0 && k < dense_len)
			dense[k] = nation[i];
	}
}

hipError_t
launch_cust_dense_fill_nat(hipStream_t s, const int64_t *custkey,
			   const uint8_t *nation, int64_t n, uint8_t *dense,
			   int64_t dense_len)
{
	hipLaunchKernelGGL(k_cust_dense_fill_nat, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, custkey, nation, n, dense,
			   dense_len);
	return hipGetLastError();
}

/* count-helper launchers used by engine_abi.cpp */
hipError_t
launch_count_filter_u8(hipStream_t s, const uint8_t *col, uint8_t val,
		       int64_t n, unsigned long long *out)
{
	hipLaunchKernelGGL(k_count_filter_u8, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, col, val, n, out);
	return hipGetLastError();
}

hipError_t
launch_count_orders_match(hipStream_t s, const int64_t *ckey,
			  const int32_t *odate, int64_t n, int32_t cutoff,
			  DeviceHashTable cust, const unsigned long long *cust_bits,
			  int64_t cust_dlen, unsigned long long *out)
{
	hipLaunchKernelGGL(k_count_orders_match, dim3(grid_for(n)),
			   dim3(THREADS), 0, s, ckey, odate, n, cutoff,
			   cust.keys, cust.nslots, cust.bloom,
			   cust.bloom_words, cust_bits, cust_dlen, out);
	return hipGetLastError();
}

}				/* namespace gg */
