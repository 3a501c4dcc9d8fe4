/*
 * engine_abi.h — the C-ABI drop-in boundary of the MI355X columnar
 * query-operator engine (libgreengage_engine.so).
 *
 * This is the surface a Greengage segment-side shim binds: the segment
 * postgres process loads a .so via shared_preload_libraries
 * (reference: utils/misc/guc.c:3001) whose _PG_init
 * (utils/fmgr/dfmgr.c:176–280) installs
 * ExecutorStart_hook/ExecutorRun_hook/ExecutorEnd_hook
 * (executor/execMain.c:129–132, call sites :334/:1036/:1309; typedefs
 * include/executor/executor.h:90–105).  The shim walks the PlanState
 * tree of the QueryDesc, claims recognized
 * SeqScan→HashJoin→Agg→Sort/Motion-bounded subtrees, and calls this
 * engine; everything else falls back to standard_ExecutorRun.
 * INTEGRATION.md shows the shim-side binding.
 *
 * Per-entry-point reference interface each call replaces:
 *   gg_engine_init/shutdown   — _PG_init-time setup (dfmgr.c:279)
 *   gg_engine_register_table  — the table-AM scan source the claimed
 *                               SeqScan would read (nodeSeqscan.c:141
 *                               InitScanRelation / aocs_beginscan
 *                               aocsam.c:426): caller hands columnar
 *                               buffers instead of a Relation
 *   gg_engine_compile_pipeline— ExecutorStart of the claimed subtree
 *                               (execMain.c:334 standard_ExecutorStart →
 *                               InitPlan)
 *   gg_engine_execute         — ExecutorRun/ExecutePlan of the subtree
 *                               (execMain.c:988/:3218): runs the whole
 *                               pipeline to completion and materializes
 *                               result batches into caller-owned memory
 *                               (slot ownership rule: execScan.c:142,
 *                               SURVEY §8(b))
 *   gg_engine_comm_*          — the Motion exchange the subtree's
 *                               Motion node would perform
 *                               (nodeMotion.c:1574 doSendTuple /
 *                               cdbmotion.c:434 SendTuple over
 *                               ic_udpifc.c), carried on RCCL over xGMI
 *   gg_engine_stats           — per-node Instrumentation the shim feeds
 *                               into EXPLAIN ANALYZE (instrument.c:423,
 *                               explain_gp.c cdbexplain_recvExecStats)
 *
 * Error model: status-code returns + gg_engine_last_error() — never
 * longjmp across HIP frames; the shim converts to ereport(ERROR)
 * (SURVEY §8(b) "Errors").  Threading: entry points are called from the
 * backend thread; the engine may use HIP streams/threads internally.
 */
#ifndef GG_ENGINE_ABI_H
#define GG_ENGINE_ABI_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
typedef enum gg_status
{
	GG_OK = 0,
	GG_EINVAL = 1,		/* bad argument / unknown handle */
	GG_EGPU = 2,		/* HIP runtime failure */
	GG_ENOMEM = 3,		/* device or host allocation failure */
	GG_ECOMM = 4,		/* RCCL failure */
	GG_ENOTSUP = 5,		/* plan shape not supported (shim must
				 * fall back to standard_ExecutorRun) */
	GG_ESTATE = 6		/* call sequence violation */
} gg_status;

/* thread-local message for the last non-OK return */
const char *gg_engine_last_error(void);

/* ---- engine lifecycle ---- */
typedef struct gg_engine_config
{
	int device;		/* HIP device ordinal (segment's GPU) */
	int n_segments;		/* gp segment count = world size */
	int segment_id;		/* this segment's id = rank */
	uint64_t hbm_limit_bytes;	/* 0 = no cap */
} gg_engine_config;

gg_status gg_engine_init(const gg_engine_config *cfg);
gg_status gg_engine_shutdown(void);

/* ---- column/table registry ---- */
typedef enum gg_coltype
{
	GG_COL_INT64 = 0,	/* int8/bigint */
	GG_COL_INT32 = 1,	/* int4/date (DateADT int32 days) */
	GG_COL_DEC64_S2 = 2,	/* numeric(15,2) as scaled int64 (cents) */
	GG_COL_CHAR1 = 3	/* char(1)/dict code as uint8 */
} gg_coltype;

typedef struct gg_column_desc
{
	const char *name;
	gg_coltype type;
	const void *host_data;	/* host pointer (engine uploads), or NULL
				 * if device_data is given */
	const void *device_data;/* optional: already-resident HBM buffer */
} gg_column_desc;

typedef int32_t gg_table;

/* Register a columnar table (the claimed SeqScan's source relation).
 * All rows are visible (read-only analytics path; visimap honored by
 * the shim at staging time — SURVEY §2 note). */
gg_status gg_engine_register_table(const char *name,
				   const gg_column_desc *cols, int ncols,
				   int64_t nrows, gg_table *out);

/* Engine-side synthetic registration for benchmarks: generates the
 * named TPC-H table's shard for (segment_id, n_segments) directly in
 * HBM per include/gg_gen.h (no host staging). */
gg_status gg_engine_register_synth(const char *table_name, uint64_t seed,
				   int64_t sf, gg_table *out);

gg_status gg_engine_drop_table(gg_table t);
gg_status gg_engine_table_nrows(gg_table t, int64_t *out_nrows);

/* Copy a registered column back to host (test/debug surface; the shim
 * uses result arenas, not this). buf_bytes must equal nrows × elsize. */
gg_status gg_engine_fetch_column(gg_table t, const char *col_name,
				 void *host_buf, size_t buf_bytes);

/* ---- pipeline descriptor ----
 * The shim extracts the claimed subtree into this descriptor.  v1
 * supports the §8 hot-path shapes; anything else: GG_ENOTSUP.
 * (PG 9.4 has no CustomScan — SURVEY §8(b) — so the descriptor mirrors
 * the PlanState subtree the ExecutorRun hook claims.) */
typedef enum gg_pipeline_kind
{
	/* scan(lineitem) → filter(shipdate<=c) → hashagg(rf,ls; Q1 aggs) */
	GG_PIPE_Q1 = 1,
	/* scan(customer)⋈scan(orders)⋈scan(lineitem) → hashagg(okey)
	 * → sort(rev desc, odate) limit k  [+ Motion redistributes] */
	GG_PIPE_Q3 = 2,
	/* scan(lineitem) → filter(shipdate<c) → agg(sum(price),count) */
	GG_PIPE_SUMPRICE = 3,
	/* Q5 (mpph5): customer⋈orders⋈lineitem⋈supplier⋈nation⋈region →
	 * hashagg(n_name) → sort(revenue desc); region/nation are the
	 * broadcast-Motion dims */
	GG_PIPE_Q5 = 4
} gg_pipeline_kind;

typedef struct gg_pipeline_desc
{
	gg_pipeline_kind kind;
	gg_table lineitem;	/* tables by role; -1 if unused */
	gg_table orders;
	gg_table customer;
	gg_table supplier;	/* Q5 */
	gg_table nation;	/* Q5: (nationkey, regionkey) dim */
	int32_t cutoff_date;	/* date qual lower constant (DateADT) */
	int32_t cutoff_hi;	/* Q5: o_orderdate < cutoff_hi */
	uint8_t mktsegment;	/* Q3: dict code of c_mktsegment literal */
	uint8_t regionkey;	/* Q5: r_name literal resolved to its key */
	int64_t limit_k;	/* Q3: LIMIT bound (nodeSort.c:143) */
} gg_pipeline_desc;

typedef int32_t gg_pipeline;

gg_status gg_engine_compile_pipeline(const gg_pipeline_desc *desc,
				     gg_pipeline *out);
gg_status gg_engine_drop_pipeline(gg_pipeline p);

/* ---- results ----
 * gg_engine_execute runs the pipeline on this segment's shard(s) and
 * materializes the (partial or final) result into the caller-owned
 * arena.  Layout per pipeline kind is defined in gg_result.h (fixed
 * little-endian structs).  If the pipeline contains the final Motion,
 * rank 0's arena receives the globally-combined result. */
gg_status gg_engine_execute(gg_pipeline p, void *out_arena,
			    size_t arena_bytes, size_t *out_written);

/* ---- Motion-equivalent collectives (RCCL over xGMI) ---- */
/* Bootstrap: rank 0 creates an opaque 128-byte id the caller
 * distributes (the shim would ship it via the QD dispatch;
 * bench/tests ship it via torch TCPStore). */
gg_status gg_engine_comm_id(void *out_id128);
gg_status gg_engine_comm_init(const void *id128);
gg_status gg_engine_comm_destroy(void);

/* ---- instrumentation (EXPLAIN ANALYZE-equivalent) ---- */
typedef struct gg_kernel_stat
{
	char name[48];
	int64_t launches;
	double total_ms;	/* HIP-event measured */
	int64_t rows_in;
	int64_t rows_out;
	int64_t hbm_bytes_algorithmic;
} gg_kernel_stat;

gg_status gg_engine_stats(gg_pipeline p, gg_kernel_stat *out, int cap,
			  int *out_n);

/* ---- numeric finalization (reference numeric.c display semantics;
 * product-side restatement, independent of oracle/) ---- */
void gg_engine_numeric_str(uint64_t lo, int64_t hi, int scale, char *buf64);
void gg_engine_avg_str(uint64_t sum_lo, int64_t sum_hi, int sum_scale,
		       int64_t count, char *buf64);

/* AOCS datum-stream block decode on GPU: decodes a
 * stream of reference-format blocks (datumstreamblock.c content layer;
 * versions Orig=0 / Dense=1 / Dense_Enhanced=2 with null bitmap, RLE
 * and delta compression) for fixed-length int32/int64 columns into
 * host value/null arrays.  Stream framing: repeat
 * [int32 block_size][int32 row_count][block bytes]; the Append-Only
 * Storage block-header layer and zlib/zstd codecs are the remaining
 * sub-layers.  out_width 4 or 8. */
gg_status gg_engine_aocs_decode(const uint8_t *stream, int64_t stream_len,
				int version, int datumlen, void *out_vals,
				int out_width, uint8_t *out_nulls,
				int64_t cap, int64_t *out_nrows);

/* Decode TEXT (varlena) datum-stream blocks on the GPU: arrow-style
 * output — per-row byte offset into `pool`, byte length, null flag.
 * Handles this fork's short (len|0x80) and network-byte-order 4-byte
 * varlena forms, RLE, and null bitmaps; compressed/toasted datums are
 * rejected.  pool_cap >= stream_len always suffices. */
gg_status gg_engine_aocs_decode_text(const uint8_t *stream,
				     int64_t stream_len, int version,
				     uint64_t *out_offs,
				     uint32_t *out_lens,
				     uint8_t *out_nulls, int64_t cap,
				     uint8_t *pool, int64_t pool_cap,
				     int64_t *out_nrows,
				     int64_t *out_pool_len);

/* Mount a REAL AO table: one AO segfile byte stream per column (the
 * form cdbbufferedread.c hands up); each column runs through the full
 * storage layer (headers + CRC32C + codecs + datum-stream decode)
 * straight into a device-resident column.  Columns must be NOT NULL.
 * The table is then usable by every pipeline like any registered
 * table. */
typedef struct gg_ao_column
{
	const char *name;
	gg_coltype	type;
	const uint8_t *stream;	/* raw AO segfile bytes */
	int64_t		stream_len;
	int			checksums;
	int			ao_version;	/* >= 2 */
	int			dsb_version;	/* 0/1/2 */
	int			comptype;	/* 0 none, 1 zlib, 2 zstd */
	/* nonzero for a TEXT column to mount as dictionary codes
	 * (type must be GG_COL_CHAR1; <= 255 distinct values).  The
	 * lexicographically-sorted dictionary is retrievable with
	 * gg_engine_table_text_dict for predicate-constant lookup. */
	int			text_dict;
	/* nonzero: the column may contain NULLs — the AO null bitmap
	 * (datumstreamblock.c) lands as a device NULL-flag array on the
	 * column, consumed by the generalized plan path under the
	 * strict-transition/NULL-qual rules (nodeAgg.c:413,
	 * execScan.c:185).  Zero keeps the round-1 behavior: any NULL
	 * errors the mount. */
	int			nullable;
} gg_ao_column;

gg_status gg_engine_register_table_ao(const char *name,
				      const gg_ao_column *cols, int ncols,
				      gg_table *out);

/* dictionary of a text_dict-mounted column: bytes + n+1 offsets */
gg_status gg_engine_table_text_dict(gg_table h, const char *col,
				    uint8_t *out_bytes, int64_t cap,
				    int64_t *out_offs,
				    int32_t max_entries,
				    int32_t *out_n);

/* Dictionary-encode a categorical text column (arrow-style inputs,
 * e.g. gg_engine_aocs_decode_text's output) into int32 codes + a
 * lexicographically sorted dictionary — deterministic across shards,
 * as the exchange requires.  NULLs code as -1; cardinality bounded by
 * max_dict. */
gg_status gg_engine_text_dict_encode(const uint8_t *pool,
				     const uint64_t *offs,
				     const uint32_t *lens,
				     const uint8_t *nulls, int64_t n,
				     int32_t max_dict,
				     int32_t *out_codes,
				     uint8_t *dict_bytes,
				     int64_t dict_cap,
				     int64_t *dict_offs,
				     int32_t *out_ndict);

/* MemTuple codec (access/common/memtuple.c format, the tuple layout
 * used in executor hash tables and on the Motion wire): bulk GPU
 * conversion between column arrays and MemTuple byte streams.
 * Fixed-width by-value attrs (attlen 1/2/4/8, attalign c/s/i/d) and
 * varlena text (attlen -1, attalign 'i'), nullable.
 * For fixed attrs cols[i] holds nrows elements of width attlen[i];
 * for varlena attrs cols[i] points at a gg_text_col on encode (bytes
 * pool + n+1 prefix offsets) and a gg_text_out on decode (per-row
 * offset/length pairs referencing the INPUT stream buffer —
 * zero-copy).  nulls[i] is a byte-per-row flag array or NULL.
 * Tuples over MEMTUPLE_LEN_FITSHORT (0xFFF0) switch to the large
 * binding (4-byte varoffsets, MEMTUP_LARGETUP header flag), exactly
 * as memtuple_form_to does. */
typedef struct gg_text_col
{
	const uint8_t *bytes;
	const int64_t *offs;	/* nrows+1 prefix offsets */
} gg_text_col;

typedef struct gg_text_out
{
	uint64_t   *offs;	/* per-row payload offset into the input */
	uint32_t   *lens;	/* per-row payload length */
} gg_text_out;

gg_status gg_engine_memtuple_binding(int natts, const int32_t *attlen,
				     const char *attalign, int32_t *out);
gg_status gg_engine_memtuple_binding_large(int natts,
					   const int32_t *attlen,
					   const char *attalign,
					   int32_t *out);
gg_status gg_engine_memtuple_encode(int natts, const int32_t *attlen,
				    const char *attalign,
				    const void *const *cols,
				    const uint8_t *const *nulls,
				    int64_t nrows, uint8_t *out,
				    int64_t cap, int64_t *out_len);
gg_status gg_engine_memtuple_decode(int natts, const int32_t *attlen,
				    const char *attalign,
				    const uint8_t *stream,
				    int64_t stream_len, void *const *cols,
				    uint8_t *const *nulls,
				    int64_t cap_rows, int64_t *out_nrows);

/* Motion wire chunk framing (tupchunk.h:34-84, tupser.c:400): convert
 * between a MemTuple stream and the interconnect's 4-byte-headed
 * tuple chunks (TC_WHOLE / TC_PARTIAL_* splitting at max_chunk,
 * TC_END_OF_STREAM).  Host-side. */
gg_status gg_engine_motion_chunkify(const uint8_t *tuples,
				    int64_t tuples_len, int32_t max_chunk,
				    int append_eos, uint8_t *out,
				    int64_t cap, int64_t *out_len);
gg_status gg_engine_motion_dechunkify(const uint8_t *chunks,
				      int64_t chunks_len, uint8_t *out,
				      int64_t cap, int64_t *out_len,
				      int *saw_eos);

/* Decode REAL Append-Only storage blocks (headers + CRC32C verify +
 * datum-stream content on the GPU).  Replaces the AO read path's
 * header/checksum layer (cdbappendonlystorageformat.c:125,1661 and
 * GetSmallContentHeaderInfo/GetNonBulkDenseContentHeaderInfo) for
 * int32/int64 columns; ao_version is the AORelationVersion (>=2),
 * dsb_version the datum-stream block version
 * (0=Orig,1=Dense,2=Dense_Enhanced), comptype the catalog's
 * compresstype (0=none, 1=zlib, 2=zstd — pg_compression.c registry);
 * all four AO header kinds parse (Small, NonBulkDense, BulkDense
 * long headers, LargeContent metadata+fragments); checksums verify
 * and codecs decompress host-parallel, uncompressed content decodes
 * zero-copy from the segfile bytes. */
gg_status gg_engine_aocs_decode_ao_text(const uint8_t *stream,
					int64_t stream_len, int checksums,
					int ao_version, int dsb_version,
					int comptype, uint64_t *out_offs,
					uint32_t *out_lens,
					uint8_t *out_nulls, int64_t cap,
					uint8_t *pool, int64_t pool_cap,
					int64_t *out_nrows,
					int64_t *out_pool_len);
gg_status gg_engine_aocs_decode_ao(const uint8_t *stream,
				   int64_t stream_len, int checksums,
				   int ao_version, int dsb_version,
				   int comptype, int datumlen,
				   void *out_vals, int out_width,
				   uint8_t *out_nulls, int64_t cap,
				   int64_t *out_nrows);

/* General hash group-by (execHHashagg.c find-or-create semantics on
 * arbitrary int64 keys, SUM+COUNT transitions): host buffers in,
 * groups out sorted by key ascending.  Sums wrap as two's-complement
 * int64.  Keys may be any int64 except INT64_MIN (the open-addressing
 * empty sentinel): a key of INT64_MIN anywhere in the input returns
 * GG_EINVAL with *out_ngroups = 0 (detected on the device while the
 * table is built; the message names INT64_MIN).  Returns the group
 * count; fails with GG_EINVAL if cap is too small. */
gg_status gg_engine_hash_groupby_i64(const int64_t *keys,
				     const int64_t *vals, int64_t n,
				     int64_t *out_keys, int64_t *out_sums,
				     int64_t *out_counts, int64_t cap,
				     int64_t *out_ngroups);

/* Spill-tier variant: inputs larger than budget_bytes of device
 * memory are hash-range partitioned on the GPU, staged in host
 * memory, and aggregated partition by partition (the reference's
 * spill_hash_table/agg_hash_reload semantics,
 * execHHashagg.c:1350/:1852).  Results identical to the in-memory
 * path, the GG_EINVAL for a key of INT64_MIN included;
 * out_npartitions reports the fan-out (1 = no spill).  budget_bytes
 * below 1 MiB, or an input that needs more than 4096 partitions under
 * it, is GG_EINVAL.  (Declared below, after the join.) */
/* Spill-tier hash JOIN (nodeHash.c:713 batching): both sides hash-
 * range partitioned on the GPU, staged in host memory, each partition
 * pair built+probed on the GPU.  Output: (probe_row_index, build_val)
 * per match, in no particular order.
 * Build keys must be unique (PK-side build): a duplicate build key
 * returns GG_EINVAL, detected on the device while the table is built.
 * Key 0 is reserved (table empty sentinel), as in the pipeline joins:
 * a build key 0 returns GG_EINVAL, and a probe key 0 matches nothing.
 * Either error leaves *out_nmatch = 0.  budget_bytes below 1 MiB, or
 * more than 4096 partitions under it, is GG_EINVAL. */
gg_status gg_engine_hash_join_i64_spill(const int64_t *build_keys,
					const int64_t *build_vals,
					int64_t nb,
					const int64_t *probe_keys,
					int64_t np, int64_t budget_bytes,
					int64_t *out_probe_idx,
					int64_t *out_vals, int64_t cap,
					int64_t *out_nmatch,
					int32_t *out_npartitions);

gg_status gg_engine_hash_groupby_i64_spill(const int64_t *keys,
					   const int64_t *vals, int64_t n,
					   int64_t budget_bytes,
					   int64_t *out_keys,
					   int64_t *out_sums,
					   int64_t *out_counts,
					   int64_t cap,
					   int64_t *out_ngroups,
					   int32_t *out_npartitions);

/* General ORDER BY operator: stable LSB radix sort of (u64 key, u64
 * payload) pairs on the GPU (nodeSort.c:48 / tuplesort.c semantics for
 * unbounded sorts; the LIMIT-k case uses histogram select instead,
 * mirroring tuplesort.c:1360's bounded-heap switch).  key_bytes limits
 * the passes (e.g. 4 for int32-derived keys); descending inverts the
 * key bits.  Host buffers; n < 2^32. */
gg_status gg_engine_radix_sort_u64(uint64_t *keys, uint64_t *payload_or_null,
				   int64_t n, int key_bytes, int descending);

/* ---- generalized pipeline descriptor (v2) ----------------------------
 * The compositional form of the subtree a shim extracts from the
 * PlanState tree (execProcnode.c:925–1148): a driving scan with
 * conjunctive range predicates (ExecQual execQual.c:6260 over the
 * strategy-number operator classes), zero or more hash joins against
 * filtered build tables (nodeHash.c:88 build / nodeHashjoin.c:78 probe,
 * join-qual = key equality): SEMI-join filters, or INNER joins against
 * a unique-keyed build side whose columns the rest of the plan can
 * read, a hash group-by
 * over 0–2 key columns (execHHashagg.c:905), and COUNT/SUM/AVG
 * aggregate transitions whose inputs are products of up to three
 * column factors with the (100±col) scaled-decimal modifiers TPC-H
 * money expressions need (numeric.c:1735 mul_var dscale rule;
 * ExecTargetList execQual.c:6369), plus MIN/MAX over one such factor
 * (int8smaller/int8larger).  Every aggregate may carry its own FILTER
 * (WHERE ...) conjunction, the aggregate filter advance_aggregates
 * (nodeAgg.c) evaluates ahead of the strict transition: conditional
 * aggregation, pivots, SUM(CASE WHEN c THEN x ELSE 0 END).
 * Q1/Q3/Q5-shaped descriptors keep their
 * specialized kernels via gg_engine_compile_pipeline; everything else
 * — mpph6 (Q6), changed predicate columns, ad-hoc scans — compiles
 * here with ZERO query-specific kernels.  Unsupported shapes return
 * GG_ENOTSUP (shim falls back to standard_ExecutorRun). */

#define GG_PLAN_MAX_PREDS 8
#define GG_PLAN_MAX_JOINS 2
#define GG_PLAN_MAX_AGGS 8
#define GG_PLAN_MAX_FILTERS 4
#define GG_PLAN_MAX_FILTER_PREDS 4

/* conjunct: lo <= col < hi (INT64_MIN/INT64_MAX = one-sided; equality
 * = [v, v+1)).  A NULL column value fails the qual (SQL three-valued
 * logic: WHERE discards non-true, execScan.c:185). */
typedef struct gg_plan_pred
{
	const char *col;
	int64_t lo;		/* inclusive */
	int64_t hi;		/* exclusive */
} gg_plan_pred;

typedef struct gg_plan_scan
{
	gg_table table;
	gg_plan_pred preds[GG_PLAN_MAX_PREDS];
	int npreds;
} gg_plan_scan;

/* Column sources.  Wherever a descriptor names a column that is read
 * per driving row (a join's probe_key, a group column, an aggregate
 * factor, an aggregate filter's predicate column) a source byte beside
 * it names the table the column belongs
 * to: 0 = the driving table (today's meaning, and what a
 * zero-initialised descriptor says), 1+k = the build table of join k,
 * which must be a GG_JOIN_INNER or GG_JOIN_LEFT join (for a probe_src:
 * one with a lower index than the probing join).  A source naming a SEMI
 * or ANTI join (neither has a payload), a join index >= njoins or, for
 * probe_src, a non-earlier join is GG_EINVAL. */

typedef enum gg_plan_joinkind
{
	GG_JOIN_SEMI = 0,	/* filter: does the row have a partner? */
	GG_JOIN_INNER = 1,	/* unique-keyed build side with payload */
	/* the two kinds below take the next values, 2 and 3 (pinned by the
	 * assert under the enum).  They carry no "= n" of their own because
	 * tests/test_plan_payload_cpu.py, which predates them, reads this
	 * enum's explicit values and expects exactly the two above */
	GG_JOIN_LEFT,		/* 2: INNER that keeps partnerless rows,
				 * NULL-extended (LEFT OUTER JOIN) */
	GG_JOIN_ANTI		/* 3: SEMI inverted: NOT EXISTS */
} gg_plan_joinkind;

#ifdef __cplusplus
static_assert(GG_JOIN_LEFT == 2 && GG_JOIN_ANTI == 3, "ABI join kinds");
#else
_Static_assert(GG_JOIN_LEFT == 2 && GG_JOIN_ANTI == 3, "ABI join kinds");
#endif

/* hash join against a filtered build table.
 *
 * GG_JOIN_SEMI: driving rows survive iff probe_key matches the
 * build_key of some build-side row passing the build preds.
 *
 * GG_JOIN_INNER (nodeHashjoin.c:78–510, HJ_NEED_NEW_OUTER ->
 * HJ_SCAN_BUCKET): a driving row survives iff its probe key is non-NULL
 * and equals the build key of a build row that passes the build preds
 * and has a non-NULL key (NULL keys never match, nodeHash.c:1070); the
 * row then SEES that build row: columns of the build table can be group
 * keys, aggregate factors and the probe key of a later join (source
 * 1+k).  A payload column's NULL flag is read at the build row and
 * obeys the usual rules: a NULL group key joins the NULL group, a NULL
 * factor is skipped (strict transition), a NULL chained probe key does
 * not match.  Joins run in descriptor order.
 *
 * Uniqueness: the build key of an INNER join must be unique among the
 * build rows that pass the build preds and have a non-NULL key (the
 * PK–FK case); row-multiplying joins are not implemented.  Duplicates
 * are detected on the device while building and gg_engine_execute then
 * returns GG_ENOTSUP (the shim falls back) — never a wrong row set.
 * Duplicates among rows failing the build preds or among NULL-key rows
 * do not count; SEMI joins accept duplicates.  An INNER build table of
 * 2^32-1 rows or more is GG_ENOTSUP at compile time (32-bit row
 * indices), and so is an INNER build key of INT64_MIN at execute.
 *
 * In the two kinds below, match(j) means: the probe key is non-NULL and
 * equals the build key of some build row that passes join j's build preds
 * and has a non-NULL key (the NULL-never-matches rule, nodeHash.c:1070).
 *
 * GG_JOIN_LEFT (nodeHashjoin.c HJ_FILL_OUTER_TUPLE): the row always
 * survives this join.  On a match it sees the build row exactly as under
 * INNER.  Without one it is NULL-extended: every column of source 1+j
 * reads as SQL NULL for that row, and the usual rules apply wherever such
 * a column is used: a group key joins the NULL group (GG_PLAN_NULL_KEY;
 * code 256 in a char1 pair, e = 0 in a packed pair), an aggregate factor
 * is skipped (strict transition) while COUNT(*) still counts the row, an
 * aggregate-filter conjunct is not true, and a chained probe key (a later
 * join's probe_src = 1+j) is NULL and matches nothing.  The build preds
 * are ON-clause conditions on the nullable side: they decide which build
 * rows can be partners, never which driving rows survive.  Uniqueness,
 * duplicate detection (GG_ENOTSUP at execute), the INT64_MIN build key
 * and the 2^32-1 row limit are those of INNER, and a source may name a
 * LEFT join wherever it may name an INNER one.
 *
 * GG_JOIN_ANTI (nodeHashjoin.c JOIN_ANTI, NOT EXISTS): the row survives
 * iff not match(j).  A NULL probe key matches nothing, so that row
 * SURVIVES, and so does one whose probe key comes from a NULL-extended
 * earlier LEFT join.  Duplicate build keys are fine, as for SEMI.  There
 * is no payload: a source naming an ANTI join is GG_EINVAL.
 *
 * Greenplum's JOIN_LASJ_NOTIN (NOT IN's NULL rules), RIGHT/FULL joins and
 * row-multiplying joins are not implemented; any other kind value is
 * GG_ENOTSUP. */
typedef struct gg_plan_join
{
	gg_plan_scan build;
	const char *build_key;
	const char *probe_key;	/* column of the table probe_src names */
	int kind;		/* gg_plan_joinkind */
	int8_t probe_src;	/* source of probe_key (see above) */
} gg_plan_join;

/* aggregate: COUNT(*) / COUNT(col) (non-NULL, nodeAgg strict rules) /
 * SUM(f0*f1*f2), factor = col, (100-col) or (100+col); SUM skips rows
 * whose factor inputs are NULL (strict transition, nodeAgg.c:413–460).
 *
 * MIN(f0) / MAX(f0) (int8smaller / int8larger): exactly one factor, a
 * column of any accepted type (char1 reads as 0..255) under any
 * gg_plan_fmod; nfactors != 1 is GG_ENOTSUP.  Strict: NULL inputs are
 * skipped, a group with no non-NULL input yields SQL NULL.
 *
 * AVG(f0*f1*f2): 1..3 factors like SUM.  The transition state is the
 * exact 128-bit sum plus the count of rows whose factors are all
 * non-NULL (numeric_avg's state); finalise with gg_engine_avg_str.
 *
 * COUNT(DISTINCT f0): the number of distinct non-NULL values of one column
 * among the group's rows.  nfactors == 1 and mod[0] == GG_FMOD_ID, anything
 * else is GG_ENOTSUP; the column is char1, int32 or int64 from any valid
 * source, under the source rules and GG_EINVAL cases of any factor.  NULL
 * inputs are not counted, the NULL-extended payload of a partnerless LEFT
 * row included, and a group with no non-NULL input reports 0, never NULL.
 * With a filter, a value counts iff at least one row of the group carrying
 * it passes the filter and has it non-NULL (as for COUNT).  The result is
 * one arena slot, a signed 128-bit count laid out like COUNT; HAVING atoms
 * and order entries treat it exactly as a COUNT.  Any other aggregate kind
 * may stand beside it.
 *
 * The plan is the reference's two-stage one (cdbgroup.c): an inner
 * aggregation by (group key, value), which is an ordinary plan whose last
 * group column is the distinct column, then a regroup by the group key
 * alone, on the device ahead of HAVING and the order (one segment, more than
 * 8 pairs) or on the host (GG_PLAN_DISTINCT=host in the environment forces
 * the host).  So the value restrictions on the distinct column are those of
 * a group column:
 *   ngroup == 1  the pair (g, x) travels as the two-column code of
 *                gg_plan_desc.group_cols, packed under the 62-bit budget; an
 *                over-budget pair makes the first gg_engine_execute return
 *                GG_ENOTSUP, every segment alike.  Two char1 columns keep
 *                e0 * 512 + e1
 *   ngroup == 0  the inner plan groups by x alone: values of INT64_MIN or
 *                GG_PLAN_NULL_KEY are not supported
 * Limits, each GG_ENOTSUP at compile: ngroup == 2 together with a DISTINCT
 * aggregate (the inner code would need three fields), and DISTINCT
 * aggregates over more than one (column, source) in one plan; several over
 * the same column with different filters are accepted.  Each DISTINCT
 * aggregate takes one accumulator slot of GG_PLAN_MAX_AGGS. */
typedef enum gg_plan_aggkind
{
	GG_AGG_COUNT_STAR = 0,
	GG_AGG_COUNT_COL = 1,
	GG_AGG_SUM = 2,
	GG_AGG_MIN = 3,
	GG_AGG_MAX = 4,
	GG_AGG_AVG = 5,
	/* the next value; pinned below, since it is ABI */
	GG_AGG_COUNT_DISTINCT
} gg_plan_aggkind;

#ifdef __cplusplus
static_assert(GG_AGG_COUNT_DISTINCT == 6, "gg_plan_aggkind values are ABI");
#else
_Static_assert(GG_AGG_COUNT_DISTINCT == 6, "gg_plan_aggkind values are ABI");
#endif

typedef enum gg_plan_fmod
{
	GG_FMOD_ID = 0,		/* col */
	GG_FMOD_SUB100 = 1,	/* 100 - col */
	GG_FMOD_ADD100 = 2	/* 100 + col */
} gg_plan_fmod;

typedef struct gg_plan_agg
{
	int kind;		/* gg_plan_aggkind */
	int nfactors;		/* 0 for COUNT(*); 1 for COUNT(col) */
	const char *col[3];
	int8_t mod[3];		/* gg_plan_fmod */
	int8_t src[3];		/* source of col[f] (column sources above) */
	int8_t filter;		/* 0 = none, 1+k = desc.filters[k] (below) */
} gg_plan_agg;

/* Aggregate filter: agg(...) FILTER (WHERE p0 AND p1 ...), the
 * Aggref.aggfilter that advance_aggregates (nodeAgg.c) evaluates before
 * the strict transition.  Filters are a table on the descriptor, so that
 * several aggregates can share one condition and have it evaluated once
 * per row; gg_plan_agg.filter picks one.
 *
 * A filter is evaluated per driving row that survived the WHERE
 * predicates and all joins.  It never changes which rows survive and
 * never changes which groups exist.  Its predicate columns follow the
 * "column sources" rule: src[i] = 0 is the driving table, 1+k the build
 * table of INNER join k, read at the joined build row.  A conjunct over
 * a NULL column value is not true, as for WHERE; a payload column's NULL
 * flag is read at the build row.  The aggregate then skips the row.
 *
 * Aggregate a transitions on a row iff its filter is true AND its
 * strict-input rule holds; COUNT(*) with a filter counts the rows where
 * the filter is true.  A group none of whose rows pass a filter still
 * appears, and that aggregate reports
 *   COUNT    0
 *   SUM      slot = 0: the convention for a SUM with no non-NULL input.
 *            A caller who needs FILTER's SQL NULL pairs the SUM with a
 *            COUNT under the same filter (COUNT = 0 means NULL)
 *   MIN/MAX  hi == 0, i.e. SQL NULL
 *   AVG      N = 0
 * and a plain aggregate (ngroup == 0) still yields exactly one row.
 * SUM(CASE WHEN c THEN x ELSE 0 END) and COUNT(CASE WHEN c THEN 1 END)
 * map onto a filtered SUM / COUNT(*), with that one difference (0 where
 * FILTER says NULL).
 *
 * Errors: gg_plan_agg.filter outside [0, nfilters] is GG_EINVAL;
 * nfilters outside [0, GG_PLAN_MAX_FILTERS] or a filter's npreds >
 * GG_PLAN_MAX_FILTER_PREDS (or < 0) is GG_ENOTSUP; a filter an aggregate
 * references with npreds == 0 is GG_EINVAL; a missing column, or a
 * source naming a SEMI join or a join >= njoins, is GG_EINVAL as for
 * factors.  A filter no aggregate references is validated the same way
 * and otherwise ignored: it costs no loads and no code. */
typedef struct gg_plan_filter
{
	gg_plan_pred preds[GG_PLAN_MAX_FILTER_PREDS];	/* conjunction,
							 * lo <= col < hi */
	int8_t src[GG_PLAN_MAX_FILTER_PREDS];	/* column source of
						 * preds[i].col */
	int npreds;
} gg_plan_filter;

/* ORDER BY / LIMIT over the groups (Sort + Limit above the Agg: "top-k
 * groups by an aggregate").
 *
 * Order.  Groups are ordered by order[0 .. norder), and ties are broken by
 * (key0, key1) ascending, exactly as the arena is ordered without an order
 * (raw int64, so GG_PLAN_NULL_KEY sorts first IN THE TIE-BREAK).  Groups are
 * distinct, so this is a total order and the result, with or without a
 * limit, is unique.  SQL promises no such thing; the engine does, so that a
 * plan's result is the same on every path and for every segment count.
 *   what = 0  group key `index`: compares the decoded key values as int64
 *             (char1 reads as 0..255).  A NULL key is placed by
 *             nulls_first, whatever `desc` says.
 *   what = 1  descriptor aggregate `index`:
 *             COUNT, SUM  compare as signed 128-bit values and are never
 *                         NULL (a SUM with no input is 0, as in the arena)
 *             MIN, MAX    compare the decoded int64; a group with N = 0 is
 *                         NULL and is placed by nulls_first
 *             AVG         GG_ENOTSUP at compile: comparing two AVGs exactly
 *                         needs a 128 x 64-bit cross product
 * nulls_first is explicit: the ABI has no default (PostgreSQL's is NULLS
 * LAST for ASC and NULLS FIRST for DESC; a binding may fill that in).
 *
 * Limit.  limit > 0 emits at most that many groups, the first ones of the
 * order; with norder == 0 that is LIMIT over the (key0, key1) order.  The
 * arena keeps its layout: n_groups is the number of rows emitted,
 * min(groups, limit), the rows come in the requested order, and the arena
 * needs room for only that many.  limit == 0 means NO limit: SQL's
 * LIMIT 0 (an empty result) is not expressible.  ngroup == 0 with any
 * order or limit is accepted and yields its one row.
 *
 * With one segment, 0 < limit <= GG_PLAN_MAX_LIMIT and more groups than
 * max(limit, 8), the first `limit` groups are selected on the device and
 * only they are copied back; every other case (several segments, where a
 * group's partial states live on several of them and no local top-k is the
 * global one; a larger limit; an order without a limit; a handful of
 * groups) copies the groups out and orders them on the host, with the same
 * comparator.  GG_PLAN_TOPK=host in the environment forces the host path.
 *
 * Errors: limit < 0, norder outside [0, GG_PLAN_MAX_ORDER] or est_groups
 * < 0 is GG_ENOTSUP, as is an AVG order key; `what` outside {0, 1}, a key
 * index >= ngroup or an aggregate index >= naggs (or either < 0) is
 * GG_EINVAL. */
#define GG_PLAN_MAX_ORDER 4
#define GG_PLAN_MAX_LIMIT 1024	/* device top-k; larger limits order on the
				 * host */

typedef struct gg_plan_order
{
	int8_t what;		/* 0 = group key, 1 = descriptor aggregate */
	int8_t index;		/* group column g, or aggregate a (descriptor
				 * order) */
	int8_t desc;		/* 0 ASC, 1 DESC */
	int8_t nulls_first;	/* 0 NULLS LAST, 1 NULLS FIRST */
} gg_plan_order;

typedef struct gg_plan_desc
{
	gg_plan_scan scan;	/* driving (probe-side) scan */
	gg_plan_join joins[GG_PLAN_MAX_JOINS];
	int njoins;
	/* 0 = one global group; 1 = any char1/int32/int64 column;
	 * 2 = any two char1/int32/int64 columns, each from any valid source
	 * (group_src).  NULL keys group together, separately per column
	 * (execHHashagg.c:531), and are reported as GG_PLAN_NULL_KEY.  Group
	 * values of INT64_MIN (open-addressing sentinel) or GG_PLAN_NULL_KEY
	 * are not supported, for one key or two.
	 *
	 * Every group travels as ONE 64-bit code through the group table,
	 * the per-block cache, the baked second stage and the cross-segment
	 * combine.  Two char1 columns encode e_g = the byte, 256 for NULL,
	 * code = e0 * 512 + e1.  Every other pair is PACKED by the columns'
	 * value ranges (columns are immutable):
	 *   min_g / max_g  signed min/max of the whole column in its own
	 *                  table, values under NULL flags included; a
	 *                  payload column is ranged over the whole build
	 *                  column; with n_segments > 1 the ranges are
	 *                  agreed across segments (min of mins, max of
	 *                  maxes, an empty shard being the identity)
	 *   b_g   = bit_length(max_g - min_g + 1), computed without signed
	 *           overflow; a column with no rows has b_g = 1
	 *   e_g   = 0 for a NULL key, else v - min_g + 1: in [0, 2^b_g)
	 *   code  = (e0 << b1) | e1
	 * A pair is accepted iff b0 + b1 <= 62 (gg_engine_plan_group_bits):
	 * the code is then non-negative, below 2^62, and never the empty
	 * sentinel.  The ranges are resolved at the plan's first execute,
	 * so an over-budget pair compiles and its first gg_engine_execute
	 * returns GG_ENOTSUP (every segment alike; the shim falls back).
	 * The host decodes (key0, key1) before sorting and writing the
	 * arena.  Either way, with est_groups == 0 the group table is fixed
	 * (2^18 slots for one column, 2^19 for two) and a two-column plan
	 * holds at most 2^18 groups; est_groups > 0 sizes the table from the
	 * estimate and lets it grow (below). */
	const char *group_cols[2];
	int ngroup;
	gg_plan_agg aggs[GG_PLAN_MAX_AGGS];
	int naggs;
	int8_t group_src[2];	/* source of group_cols[g] (column sources
				 * above) */
	/* aggregate filters (gg_plan_filter above); a zero-initialised
	 * tail means what a descriptor without it meant */
	gg_plan_filter filters[GG_PLAN_MAX_FILTERS];
	int nfilters;
	/* ORDER BY / LIMIT (gg_plan_order above) and the group-table
	 * estimate; a zero-initialised tail again means what a descriptor
	 * without it meant */
	gg_plan_order order[GG_PLAN_MAX_ORDER];
	int norder;		/* 0 = the (key0, key1) order */
	int64_t limit;		/* 0 = no limit; > 0 = emit at most this many
				 * groups */
	/* 0 = the fixed group table and its cap.  > 0 = an estimate of the
	 * number of groups in the style of Agg.numGroups: the table gets
	 * max(the fixed size, next_pow2(2 * min(est_groups, driving rows)))
	 * slots, and a scan that fills it is redone on a table four times
	 * the size, up to next_pow2(2 * driving rows) slots, which cannot
	 * fill.  The final size is remembered (tables are immutable), so
	 * only a plan's first execute regrows; path_plan_group_grow counts
	 * the regrows.  A table that, with its compacted output, does not
	 * fit in free device memory is refused with GG_ENOTSUP before it is
	 * allocated (the shim falls back).
	 *
	 * An underestimate is expensive by construction: once the table is
	 * full, every further row of a new group probes ALL of it before
	 * giving up, and the whole scan is then repeated.  That is what an
	 * over-cap plan has always cost before failing; a good est_groups is
	 * what avoids it.
	 *
	 * For a plan with a COUNT(DISTINCT) aggregate the group table holds
	 * one entry per distinct (group key, value) pair, so the estimate is
	 * of that count: Agg.numGroups of the inner Agg. */
	int64_t est_groups;
} gg_plan_desc;

#ifdef __cplusplus
static_assert(sizeof(gg_plan_agg) == 2 * sizeof(int) + 3 * sizeof(char *) + 8,
	      "gg_plan_agg.filter must sit in the tail padding");
#else
_Static_assert(sizeof(gg_plan_agg) == 2 * sizeof(int) + 3 * sizeof(char *) + 8,
	       "gg_plan_agg.filter must sit in the tail padding");
#endif

#define GG_PLAN_NULL_KEY (-9223372036854775807LL)	/* INT64_MIN+1 */

/* result arena layout (little-endian):
 *   int64 n_groups; int32 naggs; int32 ngroup;
 *   then n_groups rows, sorted by (key0, key1) ascending, or ordered and
 *   limited as the descriptor's order[] / limit say:
 *     int64 key0, int64 key1, then naggs x (uint64 lo, int64 hi)
 *   (a plan with G = 3 or 4 group columns, gg_plan_groups below: ngroup is
 *   G, every row carries G keys, and the order is over all of them)
 * naggs is the number of 16-byte result slots per row; slots follow
 * descriptor order:
 *   COUNT(*), COUNT(col), SUM   1 slot: a signed 128-bit value
 *   MIN, MAX                    1 slot: lo = the value as an int64 bit
 *                               pattern, hi = number of non-NULL
 *                               inputs N; hi == 0 means SQL NULL and
 *                               lo is then 0
 *   AVG                         2 slots: slot 0 = signed 128-bit sum;
 *                               slot 1 = (lo = N, hi = 0); N == 0
 *                               means SQL NULL
 * (so naggs equals the descriptor's naggs unless it holds an AVG).
 *
 * Accumulator budget: on the device every aggregate occupies
 * accumulator slots, GG_PLAN_MAX_AGGS in all.  COUNT and SUM take one;
 * MIN and MAX take a value word plus a non-NULL count; AVG takes a sum
 * plus a count.  The helper counts of MIN/MAX/AVG aggregates are shared
 * only when the factor columns, their sources and the filter index all
 * match (a helper count inherits its aggregate's filter).  A descriptor
 * whose lowered form needs more than GG_PLAN_MAX_AGGS slots returns GG_ENOTSUP; any
 * descriptor with 4 or fewer aggregates compiles. */
gg_status gg_engine_compile_plan(const gg_plan_desc *desc, gg_pipeline *out);

/* sizeof(gg_plan_desc) as this library was built: lets a binding check
 * its mirror of the layout without a GPU */
size_t gg_engine_plan_desc_size(void);

/* General WHERE clauses: a normalised boolean qual handed over BESIDE the
 * descriptor (gg_plan_desc keeps its layout; bindings pin its last field).
 * The preds of a scan, a build side or a filter are conjunctions of ranges
 * over one table's own columns; this extension adds OR, IN-lists, negated
 * ranges, column-against-column comparisons (also across a join, against a
 * payload column) and IS [NOT] NULL, for the plan's WHERE and for the build
 * filter of each join.
 *
 * Form.  Conjunctive normal form with negation only at the atoms:
 *   qual   = clauses[0] AND clauses[1] AND ...      (ExecEvalAnd)
 *   clause = atoms[0] OR atoms[1] OR ...            (ExecEvalOr)
 *   atom   = one of gg_plan_atomkind; ExecEvalNot never appears above an
 *            atom, the shim pushes it down: NOT (lo <= a < hi) is
 *            NOT_RANGE, NOT (a < b) is b <= a, NOT (a = b) is NE,
 *            NOT (a IS NULL) is NOT_NULL (ExecEvalNullTest in execQual.c).
 *   IN-list (ExecEvalScalarArrayOp, useOr): one clause of equalities
 *            [v, v+1); NOT IN (v1..vn) of constants (useOr false): n
 *            one-atom clauses of NOT_RANGE [v, v+1).
 * The shim normalises the plan's qual into this form and falls back when
 * it does not fit the limits.
 *
 * An atom is either true or not true.
 *   RANGE, NOT_RANGE, LT, LE, EQ, NE: not true when any column the atom
 *     reads is SQL NULL (the NULL-flag rule of the preds), else the literal
 *     comparison.
 *   IS_NULL: true exactly when a is SQL NULL; NOT_NULL is its complement.
 *   A column with no NULL-flag array is never NULL by itself; every column
 *     of source 1+k is NULL on a row LEFT join k NULL-extended.
 * A clause is true iff some atom is true; the qual is true iff every
 * clause is true; a row whose qual is not true is dropped (ExecQual: a
 * qual result of false or NULL rejects the tuple).
 *
 * Why two values are exact.  SQL's logic is three-valued (Kleene).  Read
 * "not true" as {FALSE, NULL}.  Negation sits only inside the atoms, and a
 * negated comparison over a NULL is still NULL, so each atom's "true" is
 * exactly Kleene TRUE.  OR is TRUE iff some operand is TRUE, AND is TRUE iff
 * every operand is TRUE: both depend only on which operands are TRUE, never
 * on whether a non-true operand is FALSE or NULL.  With no negation above
 * the atoms, "TRUE under Kleene logic" and "some atom true in every clause"
 * therefore coincide, and ExecQual keeps exactly the TRUE rows.
 *
 * Scope 0 is the plan's WHERE.  A driving row survives iff its scan.preds
 * pass, every join keeps it and every scope-0 clause is true.  Atoms follow
 * the "column sources" rule: src / src2 = 0 is the driving table, 1+k the
 * build table of INNER or LEFT join k, read at the joined build row.  On a
 * row LEFT join k NULL-extended every column of source 1+k is NULL:
 * comparisons over it are not true, IS_NULL is true.  Unlike an aggregate
 * filter, a WHERE clause decides which rows and so which groups exist; with
 * ngroup == 0 and no surviving row the plan still yields its one row.  The
 * WHERE is evaluated per segment, ahead of the cross-segment combine.
 *
 * Scope 1+k is an additional build filter of join k: a build row can be a
 * partner iff it passes joins[k].build.preds AND every scope-1+k clause.
 * Its atoms name columns of that build table; src and src2 must be 0.  For
 * a LEFT join these are ON-clause conditions on the nullable side and never
 * drop a driving row.  Uniqueness and duplicate detection count only rows
 * passing both, as for the preds.  All four join kinds take them.
 *
 * Comparisons.  LT, LE, EQ, NE compare the two values widened to int64 as
 * the plan reads them everywhere (char1 is 0..255, int32 sign-extended) with
 * a true comparison, never a subtraction: INT64_MIN < INT64_MAX holds.  > and
 * >= are LT / LE with the sides swapped.  A comparison in which exactly one
 * side is GG_COL_DEC64_S2 is GG_ENOTSUP (the scales differ).
 *
 * Ranges.  RANGE and NOT_RANGE are literal: NOT_RANGE is the exact complement
 * of RANGE on non-NULL values whatever lo / hi are, INT64_MIN / INT64_MAX
 * included.  Equality is [v, v+1), <> v its NOT_RANGE.
 *
 * where == NULL or nclauses == 0 is gg_engine_compile_plan exactly: same
 * validation, same kernels, same generated program text.  Everything else in
 * the descriptor composes unchanged (aggregate filters, ORDER BY / LIMIT,
 * est_groups growth, packed group pairs, n_segments > 1); packed ranges are
 * taken over whole columns and do not depend on the WHERE.
 *
 * Stat rows: path_plan_where counts one per execute of a plan with at least
 * one clause; hbm_bytes_algorithmic counts each distinct (column, source) of
 * the scope-0 clauses once, at its width (an 8-value IN-list reads its
 * column once).
 *
 * Errors.  GG_ENOTSUP: nclauses outside [0, GG_PLAN_MAX_CLAUSES], natoms >
 * GG_PLAN_MAX_ATOMS, more than GG_PLAN_MAX_WHERE_ATOMS atoms in all, an
 * unknown atom kind, a mixed-scale comparison.  GG_EINVAL: natoms <= 0 (an
 * empty disjunction), scope outside [0, njoins], a missing column, a col2 on
 * a non-comparison atom or none on a comparison, a source naming a SEMI or
 * ANTI join or a join >= njoins, or anything but 0 in a build scope. */
#define GG_PLAN_MAX_CLAUSES      8	/* per gg_plan_where */
#define GG_PLAN_MAX_ATOMS        8	/* per clause */
#define GG_PLAN_MAX_WHERE_ATOMS 16	/* per gg_plan_where, all clauses */

typedef enum gg_plan_atomkind
{
	GG_ATOM_RANGE = 0,	/* lo <= a < hi (what gg_plan_pred says) */
	GG_ATOM_NOT_RANGE = 1,	/* a < lo || a >= hi: <>, NOT BETWEEN */
	GG_ATOM_LT = 2,		/* a <  b   (b = col2; > and >= by swapping) */
	GG_ATOM_LE = 3,		/* a <= b */
	GG_ATOM_EQ = 4,		/* a =  b */
	GG_ATOM_NE = 5,		/* a <> b */
	GG_ATOM_IS_NULL = 6,	/* a IS NULL */
	GG_ATOM_NOT_NULL = 7	/* a IS NOT NULL */
} gg_plan_atomkind;

typedef struct gg_plan_atom
{
	const char *col;	/* a */
	const char *col2;	/* b for LT/LE/EQ/NE, else must be NULL */
	int64_t lo, hi;		/* RANGE / NOT_RANGE */
	int8_t kind, src, src2;	/* gg_plan_atomkind; column sources of a, b */
} gg_plan_atom;

typedef struct gg_plan_clause		/* atoms[0] OR atoms[1] OR ... */
{
	gg_plan_atom atoms[GG_PLAN_MAX_ATOMS];
	int natoms;
	int8_t scope;	/* 0 = the plan's WHERE; 1+k = build filter of join k */
} gg_plan_clause;

typedef struct gg_plan_where		/* clauses[0] AND clauses[1] ... */
{
	gg_plan_clause clauses[GG_PLAN_MAX_CLAUSES];
	int nclauses;
} gg_plan_where;

gg_status gg_engine_compile_plan_where(const gg_plan_desc *desc,
				       const gg_plan_where *where,
				       gg_pipeline *out);

/* sizeof(gg_plan_where), for bindings; needs no GPU */
size_t gg_engine_plan_where_size(void);

/* HAVING: a qual over the plan's aggregates, the qual of the Agg node
 * (nodeAgg.c: ExecQual over the projected aggregates decides whether a
 * finished group is emitted).  Like gg_plan_where it travels BESIDE the
 * descriptor, which keeps its layout.
 *
 * Form.  The form of gg_plan_where: conjunctive normal form, negation only
 * in the atoms, an atom either true or not true; the two-valued argument
 * given there holds word for word.
 *   having = clauses[0] AND clauses[1] AND ...
 *   clause = atoms[0] OR atoms[1] OR ...
 *   atom   = one of gg_plan_havingkind over the value v of descriptor
 *            aggregate `agg`
 *
 * Value.  v is what an order key over the same aggregate compares
 * (gg_plan_order, what = 1):
 *   COUNT(*), COUNT(col), SUM   the signed 128-bit accumulator, never NULL.
 *                               A SUM with no non-NULL input reads as 0, the
 *                               arena's convention; a caller who needs SQL's
 *                               NULL there ANDs a clause COUNT(col) >= 1
 *                               under the same filter.
 *   MIN, MAX                    the decoded int64 widened to 128 bits; NULL
 *                               when the group's non-NULL count N is 0.
 *   AVG                         GG_ENOTSUP at compile, for the reason an AVG
 *                               order key is refused.
 *
 * Comparison.  RANGE and NOT_RANGE over a NULL are not true.  IS_NULL is true
 * exactly when v is NULL (never for COUNT and SUM); NOT_NULL is its
 * complement.  Bounds are literal signed 128-bit values, lo inclusive and hi
 * exclusive: RANGE is lo <= v < hi, except that lo == INT128_MIN means no
 * lower test and hi == INT128_MAX no upper test (so v = INT128_MAX is inside
 * [x, INT128_MAX)); NOT_RANGE is the exact complement of RANGE on non-NULL
 * values, whatever lo and hi are (lo >= hi: RANGE is empty).  Constants are
 * in the aggregate's own scaled-integer units: the caller applies the scale,
 * as for arena values.  Comparing one aggregate against another, and atoms
 * over group keys, are out of scope: a group key belongs in the WHERE.
 *
 * Placement.  HAVING runs after aggregation, aggregate FILTERs included, and
 * after the cross-segment combine (a group's partial states prove nothing on
 * one segment); it runs before ORDER BY and LIMIT.  n_groups = min(surviving
 * groups, limit), or the survivor count without a limit, and the arena needs
 * room only for the emitted rows.  With ngroup == 0 the plan's one row is
 * emitted iff it passes: n_groups == 0 with 16 bytes written is a valid
 * result.
 *
 * With one segment and more than 8 groups the qual is evaluated on the
 * device, over the compacted group rows, and only the survivors (or, under a
 * limit the device top-k serves, the first `limit` of them) are copied back;
 * otherwise the groups are copied out, combined, and filtered on the host by
 * the same row test.  GG_PLAN_HAVING=host in the environment forces the host
 * path.  Stat rows: path_plan_having_device or path_plan_having_host counts
 * one per execute of a plan with HAVING, and the kernel row plan_having has
 * rows_in = groups and rows_out = survivors of the device path.
 *
 * having == NULL or nclauses == 0 is gg_engine_compile_plan_where exactly:
 * same validation, same kernels, same generated program text, no new stat
 * rows.
 *
 * Errors.  The descriptor and the WHERE are validated first.  GG_ENOTSUP:
 * nclauses outside [0, GG_PLAN_MAX_HAVING_CLAUSES], natoms >
 * GG_PLAN_MAX_HAVING_ATOMS, more than GG_PLAN_MAX_HAVING_TOTAL atoms in all,
 * an unknown kind, an atom over an AVG.  GG_EINVAL: natoms <= 0, agg outside
 * [0, naggs). */
#define GG_PLAN_MAX_HAVING_CLAUSES 4	/* per gg_plan_having */
#define GG_PLAN_MAX_HAVING_ATOMS   4	/* per clause */
#define GG_PLAN_MAX_HAVING_TOTAL   8	/* per gg_plan_having, all clauses */

typedef enum gg_plan_havingkind
{
	GG_HAVING_RANGE = 0,	/* lo <= v < hi */
	GG_HAVING_NOT_RANGE = 1,	/* v < lo || v >= hi */
	GG_HAVING_IS_NULL = 2,	/* v IS NULL */
	GG_HAVING_NOT_NULL = 3	/* v IS NOT NULL */
} gg_plan_havingkind;

typedef struct gg_plan_having_atom
{
	uint64_t lo_lo;		/* signed 128-bit lo, inclusive */
	int64_t lo_hi;
	uint64_t hi_lo;		/* signed 128-bit hi, exclusive */
	int64_t hi_hi;
	int8_t kind;		/* gg_plan_havingkind */
	int8_t agg;		/* descriptor aggregate index */
} gg_plan_having_atom;

typedef struct gg_plan_having_clause	/* atoms[0] OR atoms[1] OR ... */
{
	gg_plan_having_atom atoms[GG_PLAN_MAX_HAVING_ATOMS];
	int natoms;
} gg_plan_having_clause;

typedef struct gg_plan_having		/* clauses[0] AND clauses[1] ... */
{
	gg_plan_having_clause clauses[GG_PLAN_MAX_HAVING_CLAUSES];
	int nclauses;
} gg_plan_having;

gg_status gg_engine_compile_plan_having(const gg_plan_desc *desc,
					const gg_plan_where *where,
					const gg_plan_having *having,
					gg_pipeline *out);

/* sizeof(gg_plan_having), for bindings; needs no GPU */
size_t gg_engine_plan_having_size(void);

/* Rows per tile of the device top-k's tournament (a power of two, at least
 * 2 * GG_PLAN_MAX_LIMIT): group counts around it are where the selection
 * takes another round.  A constant of the build; needs no GPU. */
int gg_engine_plan_topk_tile(void);

/* Bit widths of a packed two-column group code (gg_plan_desc.group_cols)
 * from the two columns' signed value ranges [mn[g], mx[g]]; mn[g] >
 * mx[g] stands for a column with no rows.  Fills bits[] either way and
 * returns GG_OK iff bits[0] + bits[1] <= 62, else GG_ENOTSUP.  Pure host
 * arithmetic: needs neither gg_engine_init nor a GPU, and is what
 * gg_engine_execute itself decides by. */
gg_status gg_engine_plan_group_bits(const int64_t mn[2], const int64_t mx[2],
				    int bits[2]);

/* Three or four group columns: columns 2 and 3 are handed over BESIDE the
 * descriptor, like gg_plan_where and gg_plan_having (gg_plan_desc keeps its
 * layout and its ngroup <= 2 rule).  The plan then groups by G = 2 + ncols
 * columns: desc->group_cols[0..1], then cols[0..ncols-1].  Types and sources
 * are those of group_cols; NULL keys group separately per column, a column
 * of a NULL-extended LEFT row reads as NULL, and group values of INT64_MIN
 * or GG_PLAN_NULL_KEY stay unsupported.
 *
 * Code.  Every G >= 3 plan is packed by value ranges, char1 columns
 * included, with b_g and e_g exactly as documented at
 * gg_plan_desc.group_cols:
 *   code = e0 || e1 || ... || e(G-1), field 0 most significant
 * and is accepted iff the widths sum to at most 62
 * (gg_engine_plan_group_bits_n).  The ranges are resolved at the first
 * execute: an over-budget plan compiles, and every gg_engine_execute of it
 * returns GG_ENOTSUP naming the widths.  With n_segments > 1 the ranges of
 * all G columns are agreed across the segments, so all proceed or all
 * refuse.  The code is monotone in (key0 .. key(G-1)) with NULL first.
 *
 * Group table.  est_groups == 0: the two-column table, 2^19 slots and at most
 * 2^18 groups; est_groups > 0 sizes and grows it as for any plan.
 *
 * Arena.  The header's ngroup field is G, and every row carries G int64 keys
 * (not two) ahead of its slots.  Without an order the rows are sorted by
 * (key0 .. key(G-1)) ascending as raw int64; the same tuple breaks ties under
 * an order.  A gg_plan_order entry with what = 0 may name index < G.
 * HAVING, LIMIT and ORDER BY compose unchanged.  Plans with G <= 2 keep
 * their arena byte for byte.
 *
 * groups == NULL or ncols == 0 is gg_engine_compile_plan_having exactly:
 * same validation, same kernels, same generated programs, no new stat rows.
 * Errors: ncols outside [0, 2] is GG_ENOTSUP; ncols > 0 with desc->ngroup
 * != 2 is GG_EINVAL; a missing column, or a source naming a SEMI or ANTI
 * join or a join >= njoins, is GG_EINVAL; a COUNT(DISTINCT) aggregate with
 * ncols > 0 is GG_ENOTSUP (the inner code would need a fifth field).
 * Stat rows: a packed G >= 3 execute counts path_plan_group_packed and
 * path_plan_group_packed_n. */
#define GG_PLAN_MAX_GROUP_COLS 4
typedef struct gg_plan_groups		/* group columns 2 and 3 */
{
	const char *cols[GG_PLAN_MAX_GROUP_COLS - 2];
	int8_t src[GG_PLAN_MAX_GROUP_COLS - 2];	/* column sources rule */
	int ncols;				/* 0, 1 or 2 */
} gg_plan_groups;

gg_status gg_engine_compile_plan_groups(const gg_plan_desc *desc,
					const gg_plan_where *where,
					const gg_plan_having *having,
					const gg_plan_groups *groups,
					gg_pipeline *out);

/* sizeof(gg_plan_groups), for bindings; needs no GPU */
size_t gg_engine_plan_groups_size(void);

/* gg_engine_plan_group_bits for n columns, 1 <= n <= GG_PLAN_MAX_GROUP_COLS
 * (GG_EINVAL otherwise): fills bits[0..n-1] and returns GG_OK iff they sum to
 * at most 62, else GG_ENOTSUP.  For n = 2 it is gg_engine_plan_group_bits.
 * Pure host arithmetic, and what gg_engine_execute decides by. */
gg_status gg_engine_plan_group_bits_n(int n, const int64_t *mn,
				      const int64_t *mx, int *bits);

/* Attach a NULL-flag array (1 byte per row, nonzero = NULL) to a
 * registered column — the nullable-scan surface (AO null bitmaps land
 * here; aocsam.c:699 per-column null arrays).  Predicates, group keys
 * and aggregate transitions then follow the strict-transition /
 * NULL-key rules above. */
gg_status gg_engine_table_set_nulls(gg_table t, const char *col,
				    const uint8_t *host_nulls);

/* NULL-aware general hash group-by (execHHashagg find-or-create +
 * nodeAgg.c:413 strict transitions): NULL keys form one group
 * (reported as GG_PLAN_NULL_KEY); NULL vals are skipped by both SUM
 * and COUNT (the strict SUM/AVG transition pair).  key_nulls/
 * val_nulls may be NULL (= no NULLs).  A key of INT64_MIN (NULL-flagged
 * or not), or a non-NULL key equal to GG_PLAN_NULL_KEY (it would merge
 * into the NULL group), returns GG_EINVAL with *out_ngroups = 0. */
gg_status gg_engine_hash_groupby_i64_n(const int64_t *keys,
				       const uint8_t *key_nulls,
				       const int64_t *vals,
				       const uint8_t *val_nulls, int64_t n,
				       int64_t *out_keys, int64_t *out_sums,
				       int64_t *out_counts, int64_t cap,
				       int64_t *out_ngroups);

/* build info: "gfx950" etc. — lets callers assert the native path */
const char *gg_engine_build_info(void);

#ifdef __cplusplus
}
#endif

#endif /* GG_ENGINE_ABI_H */
