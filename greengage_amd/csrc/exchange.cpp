/*
 * Inter-segment exchange helpers shared by the hand-written pipelines
 * (engine_abi.cpp) and the compiled plans (plan.cpp): the host-to-host
 * allgather and one Motion redistribute leg, both over comm.cpp's RCCL
 * collectives and the pipeline's grow-only named scratch.
 */
#include <string>
#include <vector>

#include "engine_internal.h"

namespace gg
{

/* Allgather `count` words per segment into all[count * nseg], rank-major.
 * The words are staged in the named scratch buffer (count + count * nseg
 * words); `from` says where `mine` lives: a device-resident source (an
 * accumulator) is copied device-to-device, never through the host. */
gg_status
allgather_host_u64(Pipeline *p, const char *scratch,
		   const unsigned long long *mine, size_t count,
		   std::vector<unsigned long long> &all, hipMemcpyKind from)
{
	const size_t nseg = (size_t) engine().cfg.n_segments;
	unsigned long long *g = (unsigned long long *)
		p->sget(scratch, (count + count * nseg) * 8);

	if (!g)
		return fail(GG_ENOMEM, "allgather scratch %s", scratch);
	GG_HIP(hipMemcpy(g, mine, count * 8, from));
	GG_TRY(comm_allgather_u64(g, g + count, count));
	all.resize(count * nseg);
	GG_HIP(hipMemcpy(all.data(), g + count, all.size() * 8,
			 hipMemcpyDeviceToHost));
	return GG_OK;
}

/* One Motion redistribute leg (doSendTuple routing, nodeMotion.c:1600–1636,
 * bit-exact cdbhash): partition the n rows by `key`, scatter up to three
 * int64 columns (a nullptr slot is unused) into per-destination send
 * buffers, exchange the count vector, and alltoallv every column.
 * out[c] receives column c's rows (nullptr for an unused slot), *nrecv their
 * number.  Send and receive buffers are named after `tag`, so the output of
 * one leg stays live while the next leg of the same query scatters; the
 * small count and offset vectors are shared by all legs. */
gg_status
motion_redistribute(Pipeline *p, const int64_t *key,
		    const int64_t *const in[3], int64_t n, const char *tag,
		    int64_t *out[3], uint64_t *nrecv)
{
	Engine &e = engine();
	const int nseg = e.cfg.n_segments, me = e.cfg.segment_id;
	unsigned long long *dcnt =
		(unsigned long long *) p->sget("dcnt", (size_t) nseg * 8);
	unsigned long long *doffs =
		(unsigned long long *) p->sget("doffs", (size_t) nseg * 8);
	std::vector<unsigned long long> cnts(nseg), offs(nseg + 1, 0);
	int64_t *send[3] = {nullptr, nullptr, nullptr};

	if (!dcnt || !doffs)
		return fail(GG_ENOMEM, "exchange scratch");
	GG_HIP(hipMemsetAsync(dcnt, 0, (size_t) nseg * 8, e.stream));
	GG_HIP(launch_part_count(e.stream, key, n, nseg, dcnt));
	GG_HIP(hipStreamSynchronize(e.stream));
	GG_HIP(hipMemcpy(cnts.data(), dcnt, (size_t) nseg * 8,
			 hipMemcpyDeviceToHost));
	for (int i = 0; i < nseg; i++)
		offs[i + 1] = offs[i] + cnts[i];

	for (int c = 0; c < 3; c++)
	{
		if (!in[c])
			continue;
		std::string nm = std::string(tag) + ".s" + (char) ('0' + c);

		send[c] = (int64_t *) p->sget(nm.c_str(), ((size_t) n + 1) * 8);
		if (!send[c])
			return fail(GG_ENOMEM, "send scratch %s", nm.c_str());
	}
	GG_HIP(hipMemcpy(doffs, offs.data(), (size_t) nseg * 8,
			 hipMemcpyHostToDevice));
	GG_HIP(launch_part_scatter3(e.stream, key, n, nseg, in[0], in[1],
				    in[2], doffs, send[0], send[1], send[2]));
	GG_HIP(hipStreamSynchronize(e.stream));

	/* exchange the count vector, derive the receive layout: segment s
	 * sends me allcnt[s][me] rows */
	std::vector<unsigned long long> allcnt;
	std::vector<unsigned long long> rcnts(nseg), roffs(nseg + 1, 0);

	GG_TRY(allgather_host_u64(p, "cntg", cnts.data(), (size_t) nseg,
				  allcnt));
	for (int s = 0; s < nseg; s++)
		rcnts[s] = allcnt[(size_t) s * nseg + me];
	for (int i = 0; i < nseg; i++)
		roffs[i + 1] = roffs[i] + rcnts[i];
	*nrecv = roffs[nseg];

	for (int c = 0; c < 3; c++)
	{
		out[c] = nullptr;
		if (!in[c])
			continue;
		std::string nm = std::string(tag) + ".r" + (char) ('0' + c);

		out[c] = (int64_t *) p->sget(nm.c_str(), (*nrecv + 1) * 8);
		if (!out[c])
			return fail(GG_ENOMEM, "recv scratch %s", nm.c_str());
	}
	for (int c = 0; c < 3; c++)
		if (in[c])
			GG_TRY(comm_alltoallv_i64(send[c], offs.data(),
						  cnts.data(), out[c],
						  roffs.data(), rcnts.data()));
	return GG_OK;
}

}				/* namespace gg */
