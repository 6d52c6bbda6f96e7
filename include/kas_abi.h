/*
 * kas_abi.h — C ABI of the MI355X batch solver for kafka-assigner's minimal-movement,
 * rack-aware rebalance path.
 *
 * This is the drop-in boundary for exactly one reference call site:
 *
 *   KafkaTopicAssigner.generateAssignment            KafkaTopicAssigner.java:42-72
 *     -> KafkaAssignmentStrategy.getRackAwareAssignment
 *                                                     KafkaAssignmentStrategy.java:40-63
 *
 * Everything the reference passes as boxed Java collections is passed here as flat,
 * caller-owned int32 tables:
 *
 *   reference argument (KafkaAssignmentStrategy.java:40-43)     this ABI
 *   ----------------------------------------------------------  ---------------------------------
 *   String topicName                                            kas_topic_desc.name_hash
 *                                                               (= topicName.hashCode(); only use
 *                                                               of the name is KAS:190)
 *   Map<Integer,List<Integer>> currentAssignment                cur pool: cur[P][cur_width] broker
 *                                                               ids, rows in ascending partition
 *                                                               id order (+ optional cur_len[P])
 *   Map<Integer,String> nodeRackAssignment                      node_rack[N] dense rack index
 *                                                               (rack-less broker = own unique
 *                                                               index, KAS:82-86)
 *   Set<Integer> nodes                                          node_id[N] strictly ascending
 *   Set<Integer> partitions                                     implicit = rows of cur; optional
 *                                                               in_partitions[P] flags for direct
 *                                                               callers that pass a different set
 *   int replicationFactor                                       kas_topic_desc.rf (resolved per
 *                                                               KafkaTopicAssigner.java:49-62)
 *   Context context                                             ctx pool: counter[N][ctx_width]
 *                                                               (KAS:360-369, KAS:244-302)
 *   return Map<Integer,List<Integer>>                           out pool: out[P][out_width] broker
 *                                                               ids in preference order, -1 padded
 *   IllegalStateException (KAS:183-184, KTA:65-69)              kas_topic_result.status/.fail_partition
 *
 * The boundary is generateAssignment-level: the replication-factor preconditions of
 * KafkaTopicAssigner.java:65-69 are applied by the solver (KAS_FAIL_RF_NOT_POSITIVE /
 * KAS_FAIL_RF_GT_BROKERS), i.e. rf outside [1, N] never reaches the KAS:40-63 phases, exactly
 * as no call through KTA:70-71 can carry such an rf.  (getRackAwareAssignment itself has no such
 * checks; callers that bypass KafkaTopicAssigner see the KTA status for those two ranges.)
 *
 * A *scenario* is one cluster snapshot: one broker set + rack map and an ordered list of
 * topics that share one Context (what one `--mode PRINT_REASSIGNMENT` run of
 * KafkaAssignmentGenerator.java:131-187 solves).  A *batch* is many independent scenarios;
 * the GPU solves them concurrently, one wavefront per scenario.
 *
 * Rules: no C++ types, exceptions or longjmp cross this boundary; the library never
 * retains caller pointers after a call returns (a plan copies what it needs); every
 * function returns 0 or a negative KAS_E_* code and kas_last_error() gives thread-local
 * detail.  There is no CPU fallback: without a HIP device the solve entry points fail.
 */
#ifndef KAS_ABI_H
#define KAS_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (the front entries below — kas_front_rank_device, kas_front_device / 16, kas_solve_host_front / 16 — were added under
 * version 6 as well: purely additive) */
/* (the moves entries below — kas_moves_device / 16, kas_solve_host_moves / 16, kas_solve_host_choose_moves / 16 — were added
 * under version 6 as well: purely additive) */
/* (the choose entries below — kas_rank_device, kas_choose_device / 16, kas_solve_host_choose / 16 — were added under
 * version 6: purely additive, no existing struct, entry or behaviour changed) */
#define KAS_ABI_VERSION 6

/* Longest replica list the kernels keep in registers: max(cur_width, rf) <= KAS_MAX_WIDTH. */
#define KAS_MAX_WIDTH 8

/* ---- return codes of the entry points (negative = call failed) ------------------------ */
#define KAS_E_OK            0
#define KAS_E_INVALID_ARG  (-1)  /* NULL pointer, negative size, inconsistent descriptor   */
#define KAS_E_HIP          (-2)  /* a HIP runtime call failed or no gfx950 device present   */
#define KAS_E_UNSUPPORTED  (-3)  /* shape beyond what the kernels hold in LDS / registers   */
#define KAS_E_NOMEM        (-4)

/* ---- per-topic status codes (the reference's exceptions, as data) --------------------- */
#define KAS_OK                   0
#define KAS_FAIL_UNASSIGNABLE    1  /* KAS:183-184 "Partition p could not be fully assigned!";
                                       fail_partition = p                                   */
#define KAS_FAIL_RF_NOT_POSITIVE 2  /* KTA:65-66                                            */
#define KAS_FAIL_RF_GT_BROKERS   3  /* KTA:67-69                                            */
#define KAS_FAIL_HASH_INDEX      4  /* topic.hashCode()==Integer.MIN_VALUE: Math.abs stays
                                       negative -> ArrayIndexOutOfBounds at KAS:190-192      */
#define KAS_FAIL_RF_MISMATCH     5  /* KTA:58-60; raised while resolving rf on the host
                                       (kas_resolve_replication_factor, the mirrors), never by
                                       the kernels                                           */
#define KAS_SKIPPED              6  /* an earlier topic of the same scenario failed; the CLI
                                       run would have aborted (KAG:173-184)                  */
#define KAS_FAIL_BAD_NODES       7  /* node_id[] not strictly ascending (KAS:80 analogue),
                                       a negative node id (-1 is the pad value of out rows;
                                       Kafka broker ids are non-negative), or node_rack[]
                                       outside [0, 32767]                                    */

#define KAS_FAIL_WATCHDOG        8  /* internal error, reported instead of a hung GPU: a wavefront
                                       polled KAS_SPIN_BOUND times (2^25: seconds) for another
                                       wavefront of its workgroup without progress; the scenario's
                                       rows are unspecified.  No input is known to cause it.  (Fill
                                       kernel and order kernels for lists <= 3 wide; the wide form
                                       carries the bound in test builds only)                      */

/* One topic of one scenario.  Offsets are in int32 elements into the named pool. */
typedef struct kas_topic_desc {
  int32_t name_hash;        /* Java String.hashCode() of the topic name (KAS:190)           */
  int32_t n_partitions;     /* P = number of rows of cur (= |keys(currentAssignment)|)      */
  int32_t cur_width;        /* columns of the cur table (longest current replica list)      */
  int32_t rf;               /* replication factor handed to KAS:40-43                       */
  int32_t out_width;        /* columns of the out table, >= max(cur_width, rf)              */
  int32_t reserved;
  int64_t cur_off;          /* cur pool: cur[P][cur_width], row-major, broker ids            */
  int64_t out_off;          /* out pool: out[P][out_width]                                   */
  int64_t cur_len_off;      /* aux pool: int32 len[P] (ragged lists), or -1 = all full width */
  int64_t in_partitions_off;/* aux pool: int32 flag[P] (row is in `partitions`), or -1 = all */
  int64_t part_id_off;      /* aux pool: ascending int32 partition ids[P], or -1 = 0..P-1    */
} kas_topic_desc;

/* One scenario = one broker set and an ordered run of topics sharing one Context. */
typedef struct kas_scenario_desc {
  int32_t n_nodes;          /* N                                                             */
  int32_t topic_begin;      /* first topic (index into the topic descriptor array)           */
  int32_t topic_count;      /* topics solved in this order against one Context               */
  int32_t ctx_width;        /* columns of the Context counter table (0 = no Context in/out)  */
  int64_t node_off;         /* node pools: node_id[N] (strictly ascending) and node_rack[N]  */
  int64_t ctx_off;          /* ctx pool: counter[N][ctx_width] read at start, written at end;
                               -1 = start from an empty Context and do not write it back     */
} kas_scenario_desc;

/* Per-topic outcome (what one generateAssignment call would have returned/thrown). */
typedef struct kas_topic_result {
  int32_t status;           /* KAS_OK or a KAS_FAIL_* / KAS_SKIPPED code                     */
  int32_t fail_partition;   /* partition id for KAS_FAIL_UNASSIGNABLE, else -1               */
  int32_t moved_replicas;   /* sum_p |set(new[p]) \ set(cur[p])|                             */
  int32_t moved_partitions; /* #{p : set(new[p]) != set(cur[p])}                             */
} kas_topic_result;

/* Per-scenario record: fixed 32 bytes, the unit of the multi-GPU all-gather. */
typedef struct kas_scenario_result {
  int32_t  status;          /* status of the first failing topic, or KAS_OK                  */
  int32_t  fail_topic;      /* index of that topic within the scenario, or -1                */
  int32_t  fail_partition;  /* its fail_partition, or -1                                     */
  int32_t  moved_replicas;  /* summed over the scenario's solved topics                      */
  int32_t  moved_partitions;
  int32_t  reserved;
  uint64_t digest;          /* order-independent 64-bit checksum of every emitted
                               (topic, partition row, replica slot, broker id); see
                               kas_digest_cell()                                             */
} kas_scenario_result;

/* Host view of a batch: descriptors and node tables always live in HOST memory (a plan
 * uploads them once); the bulk tables are passed separately per solve so they can be
 * device resident. */
typedef struct kas_batch_desc {
  int32_t n_scenarios;
  int32_t n_topics;
  const kas_scenario_desc* scenarios;   /* [n_scenarios]                                     */
  const kas_topic_desc*    topics;      /* [n_topics]                                        */
  const int32_t* node_id;               /* node pool, host                                   */
  const int32_t* node_rack;             /* rack pool, host (same offsets as node_id)         */
  int64_t node_pool_len;                /* elements in each node pool                        */
} kas_batch_desc;

/* Bulk tables of one solve.  All pointers are DEVICE pointers for kas_solve_device and
 * HOST pointers for kas_solve_host.  aux/ctx may be NULL when no descriptor refers to them. */
typedef struct kas_tables {
  const int32_t* cur;                   /* cur pool                                          */
  int32_t*       out;                   /* out pool                                          */
  const int32_t* aux;                   /* cur_len / in_partitions / part_id arrays          */
  int32_t*       ctx;                   /* Context counters, in/out                          */
  kas_topic_result*    topic_results;   /* [n_topics]                                        */
  kas_scenario_result* scenario_results;/* [n_scenarios]                                     */
  int64_t cur_len, out_len, aux_len, ctx_len; /* pool sizes in elements (host path copies
                                                 exactly this much; device path ignores)      */
} kas_tables;

typedef struct kas_ctx  kas_ctx;    /* device context: HIP device + stream + scratch         */
typedef struct kas_plan kas_plan;   /* validated batch shape: descriptors + node tables in HBM,
                                       launch geometry, LDS carve-up                          */

/* Contribution of one emitted cell to kas_scenario_result.digest (sum modulo 2^64 over all
 * cells).  Pure function, usable by any checker.  topic = index within the scenario,
 * row = partition row index, slot = position in the preference list. */
#ifndef KAS_ABI_FN
#define KAS_ABI_FN static inline   /* the HIP translation unit adds __host__ __device__ */
#endif
KAS_ABI_FN uint64_t kas_digest_cell(uint32_t topic, uint32_t row, uint32_t slot,
                                       int32_t broker) {
  /* one 32x32->64 multiply-add per cell: the order kernel evaluates this inside its commit path */
  const uint32_t tlo = (topic + 1u) * 0x9E3779B1u, thi = (topic + 1u) * 0x85EBCA77u;
  const uint32_t b = (uint32_t)broker ^ tlo ^ 0x7F4A7C15u;
  const uint32_t r = (((row << 4) | ((slot & 7u) << 1) | 1u)) ^ (thi & 0xFFFFFFFEu);   /* odd */
  uint64_t x = (uint64_t)b * (uint64_t)r + (((uint64_t)r << 32) | (uint64_t)b);
  x ^= x >> 29;
  return x;
}

int         kas_abi_version(void);
const char* kas_strerror(int code);          /* text for KAS_E_* return codes               */
const char* kas_status_string(int status);   /* text for KAS_OK / KAS_FAIL_* status codes   */
const char* kas_last_error(void);            /* thread-local detail of the last failure     */

/* KTA:47-69 as data (host arithmetic, no device): the replication factor generateAssignment resolves from the current
 * assignment when desiredReplicationFactor < 0, and its three precondition checks.  partition_ids[i] / list_sizes[i]: the
 * entries of currentAssignment IN THE ORDER THE CALLER'S MAP ITERATES (KTA:50: the first entry fixes the factor, KTA:57-60: the
 * first later entry of another size fails the topic).  Returns 0 and fills *res: status KAS_OK (rf = the factor to solve with),
 * KAS_FAIL_RF_MISMATCH (fail_partition, fail_list_size = the entry of KTA:58-60; rf = the factor it was held against),
 * KAS_FAIL_RF_NOT_POSITIVE (KTA:65-66) or KAS_FAIL_RF_GT_BROKERS (KTA:67-69; rf = the offending factor). */
typedef struct kas_rf_result {
  int32_t status;
  int32_t rf;
  int32_t fail_partition;   /* -1 unless KAS_FAIL_RF_MISMATCH */
  int32_t fail_list_size;   /* -1 unless KAS_FAIL_RF_MISMATCH */
} kas_rf_result;
int kas_resolve_replication_factor(const int32_t* partition_ids, const int32_t* list_sizes, int32_t n_partitions,
                                   int32_t desired_rf, int32_t n_brokers, kas_rf_result* res);

/* The message of the exception the reference throws for a topic status, character for character (what a binding puts into
 * its IllegalStateException): KAS:183-184 "Partition <p> could not be fully assigned!"; KTA:58-60 "Topic <t> has partition
 * <p> with unexpected replication factor <n>"; KTA:65-66 "Topic <t> does not have a positive replication factor!"; KTA:67-69
 * "Topic <t> has a higher replication factor (<rf>) than available brokers!".  `topic` is UTF-8.  `rf` and `list_size` are
 * read only by the statuses that print them.  Returns the length written (truncated to n - 1, always terminated), 0 for KAS_OK
 * and for statuses the reference has no message for (KAS_FAIL_HASH_INDEX is an ArrayIndexOutOfBoundsException without one). */
int kas_failure_text(const char* topic, int32_t status, int32_t fail_partition, int32_t rf, int32_t list_size, char* buf, int n);

/* Number of visible HIP devices (0 when there is none; never fails). */
int kas_device_count(void);

/* Create / destroy a device context on HIP device `device` (gfx950 required). */
int  kas_ctx_create(int device, kas_ctx** out_ctx);
void kas_ctx_destroy(kas_ctx* ctx);

/* Validate a batch shape, upload descriptors + node tables, size scratch and LDS. */
int  kas_plan_create(kas_ctx* ctx, const kas_batch_desc* batch, kas_plan** out_plan);
void kas_plan_destroy(kas_plan* plan);

/* What a solve of this plan launches, for measurement records: the instantiated kernels with
 * their template arguments (list width class W, wavefronts per scenario workgroup NW, scenarios
 * per solver wavefront G, packed counters), the form of each phase and the launch geometry, as
 * one line of text, e.g.
 *   "kas_fill_kernel<3,4>[quota] grid=1000x256 lds=32016 + kas_order_permutation_kernel +
 *    kas_order_ticket_kernel<3,2,true> grid=500x192 lds=25744"
 * Reflects the current kas_plan_set_flags state.  Returns the length written (excluding the
 * terminating NUL; truncated to n-1), or a negative KAS_E_* code. */
int kas_plan_describe(const kas_plan* plan, char* buf, int n);

/* Bytes of HBM the path must move per solve of this plan, in the plan's own cell width:
 * kas_plan_create (int32 broker ids in and out — SURVEY 8(d)'s yardstick):
 *   sum over topics 4*P*(cur_width + out_width) + sum over scenarios 8*N (+ ctx in/out);
 * kas_plan_create16 (uint16 node indices; no id table is read):
 *   sum over topics 2*P*(cur_width + out_width) + sum over scenarios 4*N (+ ctx in/out). */
int64_t kas_plan_algorithmic_bytes(const kas_plan* plan);

/* Solve with every bulk table already resident in HBM.  `hip_stream` is a hipStream_t
 * (NULL = the context's own stream).  Asynchronous: returns after enqueueing.
 * A plan owns the scratch of ONE solve (orphan lists, accept masks, scenario order, device
 * counters): it supports one solve in flight.  Solves of the same plan are therefore ordered —
 * a solve enqueued on a different stream than the plan's previous one first waits (on the device,
 * hipStreamWaitEvent) for that previous solve to finish.  Callers that want several batches in
 * flight create one plan per batch in flight (what bench.py does). */
int kas_solve_device(kas_plan* plan, const kas_tables* device_tables, void* hip_stream);

/* Block until everything enqueued on the context's own stream has finished. */
int kas_ctx_synchronize(kas_ctx* ctx);

/* Host callers (JNI / ctypes / C++ mirror / the CLI's per-topic loop, KAG:172-186): tables in HOST
 * memory in, results in HOST memory out, blocking.
 * The context keeps what repeated calls can share: its device buffers only ever grow, and the plans
 * of the most recent batch shapes are reused — a plan whose descriptors + node tables are equal byte
 * for byte is used as is, any other one is rebuilt in place over the scratch it already owns (a
 * what-if caller changes the broker sets on every call) — so a caller pays no hipMalloc / hipFree
 * after the first call of a shape.  Calls on one context are serialised.
 * Copies: a pool in memory HIP knows as pinned (kas_host_alloc, hipHostMalloc, hipHostRegister) is
 * moved by DMA straight from / to the caller's buffer; pageable memory goes through the runtime's
 * staging.  Only [first, last] element a descriptor refers to is moved in either direction.  Batches
 * whose tables are large and laid out scenario by scenario are cut into (up to three) scenario ranges, and the
 * upload of one range, the solve of the previous one and the download of the one before run
 * concurrently, on streams of their own.  On an error after work was enqueued the call drains its streams
 * before it returns (no kernel or copy is left touching the caller's memory). */
int kas_solve_host(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables);

/* The what-if form of the same call (KAG:131-187: one snapshot, many broker sets, ONE assignment
 * printed): every scenario is solved and reports its 16-byte topic records and its 32-byte scenario
 * record, but out rows come back only for the scenarios listed in select[0..n_select), packed back to
 * back in that order (per selected scenario its topics in order, P x out_width ints each;
 * host_tables->out_len >= their sum; out may be NULL when n_select == 0).  With every scenario's
 * cur_off pointing at the same rows (the layout of kafka-assigner_amd/whatif.py) a call moves one cur
 * table and the node tables up and a few kilobytes down.  n_select < 0: every row, in place, exactly as
 * kas_solve_host. */
int kas_solve_host_select(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables,
                          const int32_t* select, int32_t n_select);

/* ---- ABI v5: the same host call with 16-bit cells -------------------------------------------------------
 * The host boundary of the per-topic call (KafkaTopicAssigner.java:70-71) and of the CLI's loop over topics
 * (KafkaAssignmentGenerator.java:173-184) is bound by the host link, not by the solve; kas_solve_host16 moves half the
 * bytes.  cur / out cells are uint16 NODE INDICES: cell value i names node i of the scenario's node table — the i-th
 * smallest broker id of its broker set; every caller sorts the ids anyway to lay out node_rack[] (the reference's own
 * TreeSet at KafkaAssignmentStrategy.java:73-99), and maps cells back with one table lookup.  KAS_CELL16_NONE in cur =
 * a broker that is not in the scenario's broker set (its replica is dropped whichever broker it was, KAS:108-110), in
 * out = the pad value (-1 of the int32 layout).  Everything the algorithm derives from broker ids is their ORDER
 * (KAS:73-99 sorted nodes, KAS:188-200 processing order by position, KAS:263-278 ties by position), which the indices
 * keep: rows, statuses, fail_partition and movement counts are those of kas_solve_host on the int32 form of the same
 * batch, cell for cell after the lookup (tests/test_cells16.py).  The digest of a scenario record covers the cells as
 * emitted, i.e. kas_digest_cell over node indices.
 *   batch->node_id is not read and may be NULL (node i has id i); node_rack[], descriptors, aux, ctx, the result
 *   records and select / n_select (n_select < 0: every row in place) are exactly kas_solve_host_select's; descriptor
 *   offsets and cur_len / out_len count cells.  More than 32,767 brokers in a scenario (KAS_N_LIMIT, the limit of every plan: bit 15 of a cell means "no holder" inside the kernels): KAS_E_UNSUPPORTED.
 * On the device the batch is solved on the 16-bit cells themselves where the kernels with that I/O take it
 * (kas_plan_create16 below); any other batch is widened before and narrowed behind an int32 solve (two streaming kernels on
 * the range's solve stream). */
#define KAS_CELL16_NONE 0xFFFFu
typedef struct kas_tables16 {
  const uint16_t* cur;                  /* cur pool, node indices                            */
  uint16_t*       out;                  /* out pool, node indices                            */
  const int32_t* aux;
  int32_t*       ctx;
  kas_topic_result*    topic_results;
  kas_scenario_result* scenario_results;
  int64_t cur_len, out_len, aux_len, ctx_len;
} kas_tables16;
int kas_solve_host16(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables,
                     const int32_t* select, int32_t n_select);

/* The device-resident form of the same layout: a plan whose solves read and write 16-bit cells in HBM.  The fill kernel
 * then streams 2 bytes a cell instead of 4, the order kernel stores a final row's node indices as they are (no gather of
 * broker ids) over the mid row the row was made from, so a topic's out region is all the scratch its rows need:
 * 6 + 6 instead of 12 + 12 bytes of table traffic per row of three replicas.  Served by the kernels of lists up to 3 wide
 * (fill kernel, kas_p4_kernel, relaxation and round forms of the order kernel): any other batch — lists 4 and more wide —
 * is KAS_E_UNSUPPORTED here, and kas_solve_host16 widens such a batch on the device instead.  batch->node_id is not read; tables as kas_solve_device's, cells as kas_solve_host16's;
 * kas_plan_set_flags: no ticket form (KAS_PLAN_TICKET_ORDER takes the round form); KAS_PLAN_VERIFY_SAMPLE works as on int32 cells (round 6). */
int kas_plan_create16(kas_ctx* ctx, const kas_batch_desc* batch, kas_plan** out_plan);
int kas_solve_device16(kas_plan* plan, const kas_tables16* device_tables, void* hip_stream);

/* ---- ABI v6: per-broker movement and leadership impact, computed on the device -------------------------------
 * One streaming pass over the cur and out tables a solve used reduces every scenario to counters per broker, so that a
 * what-if caller learns what each variant does to each broker without downloading its rows.  For each scenario, over each
 * of its topics whose kas_topic_result.status == KAS_OK (failed and skipped topics contribute nothing), and each row p:
 *   C = the first clen cells of cur[p] (clen = cur_len[p], or cur_width without a cur_len array),
 *   O = the cells of out[p] up to the first pad (-1 in int32 cells, KAS_CELL16_NONE in 16-bit cells)
 * (the rows of the movement counts moved_replicas / moved_partitions).  Per node b of the scenario's node table: */
typedef struct kas_node_impact {
  int32_t replicas_before;  /* cells c of C with c == b                                       */
  int32_t replicas_after;   /* cells o of O with o == b                                       */
  int32_t leaders_before;   /* rows with clen > 0 and C[0] == b                               */
  int32_t leaders_after;    /* rows with olen > 0 and O[0] == b                               */
  int32_t inbound;          /* cells o of O with o == b that are not in C (replicas to move in) */
  int32_t outbound;         /* cells c of C with c == b that are not in O (replicas to give up) */
  int32_t reserved[2];
} kas_node_impact;

/* Per scenario (every field 0 when the scenario has no nodes): */
typedef struct kas_scenario_impact {
  int32_t departed_replicas;  /* cells of C that name no node of the scenario: a broker outside the set, or
                                 KAS_CELL16_NONE                                                    */
  int32_t leaders_moved;      /* rows with olen > 0 and (clen == 0 or O[0] != C[0])                 */
  int32_t max_inbound, max_outbound;              /* over the scenario's nodes                      */
  int32_t min_replicas_after, max_replicas_after;
  int32_t min_leaders_after, max_leaders_after;
} kas_scenario_impact;

/* Where the records go.  nodes: scenario s owns a block of n_nodes records at offset sum over s' < s of n_nodes(s'), in
 * scenario order; record i of the block is node i of the scenario's (ascending) node table.  The offset does not depend on
 * node_off: scenarios that share a node range still get blocks of their own.  scenarios: one record per scenario. */
typedef struct kas_impact_tables {
  kas_node_impact*     nodes;
  kas_scenario_impact* scenarios;
} kas_impact_tables;

/* The impact of the plan's previous solve, from the tables that solve used (device pointers, device_impact too).
 * Asynchronous, and ordered after that solve as solves of one plan are ordered (kas_solve_device); it writes every record
 * of its outputs itself.  The Sigma over nodes of inbound is the scenario record's moved_replicas.  A scenario whose
 * n_nodes x 24 bytes of counters do not fit the LDS next to the id lookup (about 6,000 brokers) counts in global scratch
 * instead: same records, up to KAS_N_LIMIT brokers.  kas_impact_device16: the same for a plan of kas_plan_create16. */
int kas_impact_device(kas_plan* plan, const kas_tables* device_tables, const kas_impact_tables* device_impact,
                      void* hip_stream);
int kas_impact_device16(kas_plan* plan, const kas_tables16* device_tables, const kas_impact_tables* device_impact,
                        void* hip_stream);

/* Exactly kas_solve_host_select / kas_solve_host16 (select, n_select as there; n_select < 0: every row in place), plus the
 * impact records in host memory.  n_select == 0: the records and the impact only, no rows come back — the what-if call. */
int kas_solve_host_impact(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables,
                          const int32_t* select, int32_t n_select, const kas_impact_tables* host_impact);
int kas_solve_host16_impact(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables,
                            const int32_t* select, int32_t n_select, const kas_impact_tables* host_impact);

/* ---- choosing the best scenarios on the device (added under ABI v6) ------------------------------------------------
 * A what-if caller compares the variants by their records and wants the rows of the best ones only.  A *criterion* is a
 * non-negative int32 taken from a scenario's kas_scenario_result and kas_scenario_impact: */
#define KAS_KEY_MOVED_REPLICAS     0  /* kas_scenario_result.moved_replicas                       */
#define KAS_KEY_MOVED_PARTITIONS   1  /* kas_scenario_result.moved_partitions                     */
#define KAS_KEY_LEADERS_MOVED      2  /* kas_scenario_impact.leaders_moved                        */
#define KAS_KEY_DEPARTED_REPLICAS  3  /* kas_scenario_impact.departed_replicas                    */
#define KAS_KEY_MAX_INBOUND        4  /* kas_scenario_impact.max_inbound                          */
#define KAS_KEY_MAX_OUTBOUND       5  /* kas_scenario_impact.max_outbound                         */
#define KAS_KEY_REPLICA_SPREAD     6  /* max_replicas_after - min_replicas_after                  */
#define KAS_KEY_LEADER_SPREAD      7  /* max_leaders_after - min_leaders_after                    */
#define KAS_KEY_MAX_REPLICAS_AFTER 8  /* kas_scenario_impact.max_replicas_after                   */
#define KAS_KEY_MAX_LEADERS_AFTER  9  /* kas_scenario_impact.max_leaders_after                    */
#define KAS_KEY_COUNT             10
#define KAS_CHOOSE_MAX_KEYS        4

/* What to rank by and how many to return.  The key of scenario s is (key[0](s), ..., key[n_keys - 1](s), s), compared
 * lexicographically, smaller is better: the scenario index makes the order total and the result deterministic.  Only
 * scenarios with kas_scenario_result.status == KAS_OK take part; n_ok is their number. */
typedef struct kas_choose_spec {
  int32_t n_keys;                       /* 1 .. KAS_CHOOSE_MAX_KEYS                                */
  int32_t key[KAS_CHOOSE_MAX_KEYS];     /* KAS_KEY_*, most significant first                       */
  int32_t k;                            /* scenarios to return, 0 <= k <= S; 0 ranks only          */
} kas_choose_spec;

/* Where a choice goes (device pointers for kas_choose_device / 16, host pointers for kas_solve_host_choose / 16):
 *   rank[S]        number of OK scenarios with a smaller key; -1 for a scenario that is not OK
 *   chosen[k]      chosen[j] = the scenario of rank j for j < min(k, n_ok), -1 for the remaining j < k
 *   row_off[k+1]   prefix sum in cells: chosen scenario j has its topics' out rows, in descriptor order, packed exactly as
 *                  kas_solve_host_select packs a selected scenario, at rows[row_off[j] .. row_off[j + 1])
 *   node_off[k+1]  the same prefix sum in records for its block of n_nodes kas_node_impact records in nodes[]
 *                  (entries of either array past min(k, n_ok) repeat the last offset)
 *   n_ok[1]
 *   rows           int32 cells (uint16 cells for the 16 forms), rows_cap cells of room
 *   nodes          nodes_cap records of room
 * Every entry of rank, chosen, row_off, node_off and n_ok is written; rows and nodes only below row_off[k] / node_off[k].
 * The arrays a call writes must not be NULL: rank (S > 0), chosen (k > 0), row_off, node_off, n_ok, and rows / nodes where
 * rows_cap / nodes_cap must be positive. */
typedef struct kas_choice {
  int32_t* rank;
  int32_t* chosen;
  int64_t* row_off;
  int64_t* node_off;
  int32_t* n_ok;
  void*    rows;
  int64_t  rows_cap;                    /* cells                                                   */
  kas_node_impact* nodes;
  int64_t  nodes_cap;                   /* records                                                 */
} kas_choice;

/* Rank n_scenarios records alone (device pointers; no plan): rank[S], chosen[spec->k] and n_ok[1] as above.  Asynchronous
 * on `hip_stream` (NULL = the context's own stream); the records must be complete on that stream. */
int kas_rank_device(kas_ctx* ctx, const kas_scenario_result* scenario_results, const kas_scenario_impact* scenario_impact,
                    int32_t n_scenarios, const kas_choose_spec* spec, int32_t* rank, int32_t* chosen, int32_t* n_ok,
                    void* hip_stream);

/* Rank the plan's previous solve and impact pass (device_tables->scenario_results, device_impact->scenarios) and gather the
 * chosen scenarios' rows (from device_tables->out) and node blocks (from device_impact->nodes) into device_choice.
 * Asynchronous, and ordered behind that solve and impact pass as kas_impact_device is ordered behind a solve — except a plan's
 * first choice, which first allocates and uploads (blocking copies) the plan's two small tables; later calls only enqueue.
 * Refused with KAS_E_INVALID_ARG before any GPU work: the spec and capacities as kas_solve_host_choose refuses them, and
 * pointers that are not aligned — rows and device_tables->out to the cell size, node records to 4 bytes, row_off / node_off
 * to 8 (the gather copies with the widest accesses the two addresses share, at least 2 bytes wide).
 * kas_choose_device16: the same for a plan of kas_plan_create16 (rows are uint16 cells). */
int kas_choose_device(kas_plan* plan, const kas_tables* device_tables, const kas_impact_tables* device_impact,
                      const kas_choose_spec* spec, const kas_choice* device_choice, void* hip_stream);
int kas_choose_device16(kas_plan* plan, const kas_tables16* device_tables, const kas_impact_tables* device_impact,
                        const kas_choose_spec* spec, const kas_choice* device_choice, void* hip_stream);

/* The what-if call that returns only the winners: the solve and the impact pass of kas_solve_host_impact for every
 * scenario; every topic record, every scenario record and every kas_scenario_impact (host_impact->scenarios) come back, and
 * so do rank[S] and chosen[k]; rows and node blocks come back for the chosen only, in host_choice.  host_tables->out and
 * host_impact->nodes are not used and may be NULL.  The ranking is over the whole call, whatever scenario ranges the call is
 * cut into.  kas_solve_host16_choose: 16-bit cells as kas_solve_host16 (rows are uint16 cells whichever cells the batch is
 * solved on).  Refused with KAS_E_INVALID_ARG before any GPU work, in this order: n_keys outside 1..4; an unknown
 * criterion; k < 0 or k > S; rows_cap below the packed size of the k largest scenarios; nodes_cap below the sum of the k
 * largest n_nodes; a NULL array that the call writes. */
int kas_solve_host_choose(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables,
                          const kas_choose_spec* spec, const kas_choice* host_choice, const kas_impact_tables* host_impact);
int kas_solve_host16_choose(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables,
                            const kas_choose_spec* spec, const kas_choice* host_choice, const kas_impact_tables* host_impact);

/* ---- the move list: a scenario's changed rows, compacted on the device (added under ABI v6) -------------------------
 * A what-if caller acts on the rows that change.  With C and O of a row exactly as the impact section above defines them
 * (the first clen cells of cur[p]; the cells of out[p] up to the first pad), and over topics whose kas_topic_result.status ==
 * KAS_OK only (failed and skipped topics contribute nothing), a row has flags: */
#define KAS_MOVE_REPLICAS 1   /* olen > 0 and set(O) != set(C)                                                  */
#define KAS_MOVE_LEADER   2   /* olen > 0 and (clen == 0 or O[0] != C[0]): the row condition of leaders_moved   */
#define KAS_MOVE_ORDER    4   /* olen > 0, set(O) == set(C), and O != C as lists                                */
/* A row with olen == 0 has no flags and is never a move.  A row is a *move under mask m* iff flags & m != 0. */
typedef struct kas_move {
  int32_t topic;      /* index of the topic within the scenario, 0 .. topic_count-1          */
  int32_t partition;  /* part_id[row], or the row index without a part_id array              */
  uint8_t flags;      /* KAS_MOVE_* of the row (all of them, not only those in the mask)     */
  uint8_t len;        /* olen                                                                 */
  uint8_t gained;     /* cells of O not in C                                                  */
  uint8_t lost;       /* cells of C not in O                                                  */
  int32_t cell_at;    /* its list is cells[cell_off[j] + cell_at .. + len)                    */
} kas_move;           /* 16 bytes */

/* Where the moves of a list of n scenarios go (device pointers for kas_moves_device / 16, host pointers for the host forms).
 * Listed scenario j owns moves[move_off[j] .. move_off[j + 1]) — its moves in (topic in descriptor order, row ascending)
 * order — and cells[cell_off[j] .. cell_off[j + 1]): their new lists, packed without pads.  move_off and cell_off are always
 * written in full and are the TRUE counts, whatever the capacities; a move is written iff its index is < moves_cap and its
 * list ends at or before cells_cap, and nothing else in moves / cells is touched: a caller learns of truncation from
 * move_off[n] > moves_cap or cell_off[n] > cells_cap.  The rows and the packed cells (sum of P x out_width) of the listed
 * scenarios are always enough room.  A list entry of -1 is an empty slot (zero moves, the offsets repeat); a scenario may be
 * listed twice, each listing gets a block of its own.  The result is deterministic: the same inputs give the same bytes.
 * Refused with KAS_E_INVALID_ARG before any GPU work: mask outside 1..7, a NULL array the call writes, pointers that are not
 * aligned (records 4 bytes, offsets 8, cells to the cell size).  A plan with a scenario whose packed cells reach 2^31 is
 * refused with KAS_E_UNSUPPORTED (cell_at is an int32). */
typedef struct kas_moves {
  int32_t  mask;      /* 1..7 */
  int32_t  reserved;
  int64_t* move_off;  /* [n+1] prefix sum of moves per listed scenario  */
  int64_t* cell_off;  /* [n+1] prefix sum of list cells                  */
  kas_move* moves;  int64_t moves_cap;   /* records */
  void*     cells;  int64_t cells_cap;   /* int32 broker ids, uint16 node indices in the 16 forms */
} kas_moves;

/* The moves of the plan's previous solve, from the tables it used.  select: a DEVICE array of n_select scenario indices (the
 * chosen[] of a kas_choice is accepted as it is, with its -1 tail).  Asynchronous, and ordered behind the plan's previous
 * solve as kas_impact_device is; a plan's first moves call allocates and uploads (blocking copies) the plan's small tables
 * and its scratch, later calls only enqueue (a list longer than any before it grows the scratch).  kas_moves_device16: the
 * same for a plan of kas_plan_create16 (cells are uint16 node indices). */
int kas_moves_device(kas_plan* plan, const kas_tables* device_tables, const int32_t* select, int32_t n_select,
                     const kas_moves* device_moves, void* hip_stream);
int kas_moves_device16(kas_plan* plan, const kas_tables16* device_tables, const int32_t* select, int32_t n_select,
                       const kas_moves* device_moves, void* hip_stream);

/* The host call that returns moves instead of rows: the batch is solved, every topic record and scenario record comes back,
 * no rows do (host_tables->out may be NULL), plus the moves of the scenarios in the HOST list select[0..n_select)
 * (n_select < 0: every scenario, in order).  The offsets are copied back first, then exactly the records that were written
 * — min(move_off[n], moves_cap) of them unless cells_cap cut the list earlier — and the cells they use, not the capacities.
 * Refusals, in this order: what kas_solve_host_select refuses; mask outside 1..7; negative capacities; a NULL array that the
 * call writes; misaligned pointers; a scenario index out of range; a scenario of 2^31 packed cells (KAS_E_UNSUPPORTED). */
int kas_solve_host_moves(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables, const int32_t* select,
                         int32_t n_select, const kas_moves* host_moves);
int kas_solve_host16_moves(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables, const int32_t* select,
                           int32_t n_select, const kas_moves* host_moves);

/* Exactly kas_solve_host_choose / 16, except that host_choice->rows may be NULL with rows_cap == 0: then no rows are gathered
 * (row_off is still the true prefix sum); with room given, rows come back as there.  The moves of the chosen come back in
 * rank order (the list is chosen[0..k)).  The 16 form returns uint16 cells whichever cells the batch is solved on.  The
 * moves refusals follow those of kas_solve_host_choose. */
int kas_solve_host_choose_moves(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables,
                                const kas_choose_spec* spec, const kas_choice* host_choice, const kas_impact_tables* host_impact,
                                const kas_moves* host_moves);
int kas_solve_host16_choose_moves(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables,
                                  const kas_choose_spec* spec, const kas_choice* host_choice, const kas_impact_tables* host_impact,
                                  const kas_moves* host_moves);

/* ---- the Pareto front of the scenarios, marked and ranked on the device (added under ABI v6: purely additive) ----------
 * A lexicographic key decides in advance that the first criterion outweighs every other.  The *front* is every scenario that
 * no other scenario beats on all criteria at once, optionally among those that respect hard bounds.
 *   eligible   scenario s is eligible iff its status is KAS_OK and limit_key[i](s) <= limit[i] for every i < n_limits.
 *   dominates  t dominates s iff both are eligible, key[i](t) <= key[i](s) for every i < n_keys, and either some
 *              key[i](t) < key[i](s) or all are equal and t < s: of scenarios with identical criteria only the earliest
 *              survives.  A strict partial order: every dominated scenario is dominated by a member.
 *   member     s is a member iff it is eligible and nothing dominates it.  A bound on a criterion among key[] only filters
 *              the front; a bound on another criterion can create members (bounds are applied before domination).
 * Members are ordered exactly as kas_choose_spec orders scenarios: (key[0], ..., key[n_keys - 1], s), lexicographic. */
#define KAS_FRONT_NOT_OK     (-1)  /* rank[s] of a scenario whose status is not KAS_OK             */
#define KAS_FRONT_OVER_LIMIT (-2)  /* ... that is OK and violates a bound                          */
#define KAS_FRONT_DOMINATED  (-3)  /* ... that is eligible and dominated                           */
typedef struct kas_front_spec {
  int32_t n_keys;                          /* 1..KAS_CHOOSE_MAX_KEYS: the criteria that are traded off   */
  int32_t key[KAS_CHOOSE_MAX_KEYS];        /* KAS_KEY_*; their order only orders the members              */
  int32_t n_limits;                        /* 0..KAS_CHOOSE_MAX_KEYS hard bounds                          */
  int32_t limit_key[KAS_CHOOSE_MAX_KEYS];  /* KAS_KEY_*, any criterion, in the spec or not                */
  int32_t limit[KAS_CHOOSE_MAX_KEYS];      /* >= 0: the criterion must be <= limit                        */
  int32_t k;                               /* members to return, 0 <= k <= S; 0 classifies only           */
} kas_front_spec;

/* A front goes into a kas_choice (above) plus int32_t counts[4] = {n_ok, n_eligible, n_front, 0}:
 *   rank[s]        for a member the number of members with a smaller key, else its class code KAS_FRONT_*
 *   chosen[j]      the member of rank j for j < min(k, n_front), -1 behind
 *   row_off[k+1], node_off[k+1]  the prefix sums over the members in that order, repeating the last offset behind
 *                  min(k, n_front), exactly as kas_choice documents them
 *   n_ok[1]        as ever; n_front > k tells the caller that the list was cut
 * Every entry of rank, chosen, the offsets, n_ok and counts is written and nothing behind them.  The same inputs give the
 * same bytes (no atomics, nothing between workgroups).
 * Refused with KAS_E_INVALID_ARG before any GPU work, in this order: n_keys outside 1..4; an unknown criterion; n_limits
 * outside 0..4; an unknown limit criterion; a negative limit; k outside 0..S; then everything the matching choose entry
 * refuses, in its order (capacities against the k largest scenarios, NULL arrays with counts among them, alignment).
 *
 * kas_front_rank_device: n_scenarios records alone (device pointers; no plan), as kas_rank_device: rank[S], chosen[k] and
 * counts[4]; scratch is n_scenarios int32 of the caller's device memory.
 * kas_front_device / 16: as kas_choose_device / 16, the front in place of the ranking; the class scratch is the plan's,
 * allocated at its first front call.
 * kas_solve_host_front / 16: kas_solve_host_choose_moves / 16 with the front in place of the ranking.  host_choice->rows ==
 * NULL with rows_cap == 0 gathers no rows; host_moves == NULL asks for no moves (kas_solve_host_choose's shape). */
int kas_front_rank_device(kas_ctx* ctx, const kas_scenario_result* scenario_results, const kas_scenario_impact* scenario_impact,
                          int32_t n_scenarios, const kas_front_spec* spec, int32_t* rank, int32_t* chosen, int32_t* counts,
                          int32_t* scratch, void* hip_stream);
int kas_front_device(kas_plan* plan, const kas_tables* device_tables, const kas_impact_tables* device_impact,
                     const kas_front_spec* spec, const kas_choice* device_choice, int32_t* counts, void* hip_stream);
int kas_front_device16(kas_plan* plan, const kas_tables16* device_tables, const kas_impact_tables* device_impact,
                       const kas_front_spec* spec, const kas_choice* device_choice, int32_t* counts, void* hip_stream);
int kas_solve_host_front(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables,
                         const kas_front_spec* spec, const kas_choice* host_choice, int32_t* counts,
                         const kas_impact_tables* host_impact, const kas_moves* host_moves);
int kas_solve_host16_front(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables,
                           const kas_front_spec* spec, const kas_choice* host_choice, int32_t* counts,
                           const kas_impact_tables* host_impact, const kas_moves* host_moves);

/* ---- rack impact: what a scenario does to racks, reduced on the device (added under ABI v6) --------------------------
 * A rack pass behind the impact pass.  Rows, C, O, clen, olen and "names a node" are exactly those of kas_node_impact above;
 * only topics whose kas_topic_result.status == KAS_OK contribute.
 *   report rack table   every scenario has an int32 table rr[i], the rack index of node i, 0 <= rr[i] < R_s with
 *                       R_s = 1 + max rr (R_s = 0 when the scenario has no nodes).  The caller may pass it as report_rack,
 *                       an array parallel to batch->node_rack (indexed by node_off + i) — so that a variant solved with
 *                       --disable_rack_awareness, whose solver table is id-as-rack, is still reported against the real
 *                       racks; NULL means the batch's own node_rack.
 *   a cell's rack       a cell that names node i has rack rr[i]; a cell of C that names no node has no rack and is not
 *                       "known".
 *   per row             kB = known cells of C, dB = distinct racks among them; kA = cells of O that name a node, dA =
 *                       distinct racks among them.
 * Ranking or fronting by these figures is not part of this pass: the scenario record is laid out (sixteen non-negative
 * int32) so that its fields are criteria of the *_racks entries below (KAS_KEY_RACK_BASE). */
#define KAS_RACK_LIMIT 4096   /* racks per scenario (the reduce kernel's R_s x 7 int32 histogram lives in the LDS) */

/* One per rack r < R_s; every field a sum over the scenario's nodes with rr == r */
typedef struct kas_rack_impact {
  int32_t nodes;              /* nodes with rr == r                                            */
  int32_t replicas_before;    /* sums of the kas_node_impact fields of the same names          */
  int32_t replicas_after;
  int32_t leaders_before;
  int32_t leaders_after;
  int32_t inbound;
  int32_t outbound;
  int32_t reserved;           /* 0 */
} kas_rack_impact;

/* Per scenario (every field 0 when the scenario has no nodes) */
typedef struct kas_scenario_rack_impact {
  /* summed over rows */
  int32_t colocated_before;         /* sum of kB - dB: replicas that share a rack with an earlier one of their row  */
  int32_t colocated_after;          /* sum of kA - dA                                                               */
  int32_t rows_colocated_before;    /* rows with kB > dB                                                            */
  int32_t rows_colocated_after;     /* rows with kA > dA                                                            */
  int32_t single_rack_rows_before;  /* rows with kB >= 2 and dB == 1                                                */
  int32_t single_rack_rows_after;   /* rows with kA >= 2 and dA == 1                                                */
  int32_t new_rack_replicas;        /* cells o of O that name a node, are not in C, and whose rack is the rack of no
                                       known cell of C                                                              */
  int32_t rows_losing_racks;        /* rows with dA < dB                                                            */
  /* taken over the scenario's racks */
  int32_t n_racks;                  /* R_s                                                                          */
  int32_t max_rack_inbound, max_rack_outbound;
  int32_t min_rack_replicas_after, max_rack_replicas_after;
  int32_t min_rack_leaders_after, max_rack_leaders_after;
  int32_t reserved;                 /* 0 */
} kas_scenario_rack_impact;

/* Where the records go.  Scenario s owns R_s rack records at racks[rack_off[s]]; rack_off[0 .. S] is the prefix sum of R_s,
 * computed on the host and returned to the caller.  racks_cap: the kas_rack_impact records `racks` has room for. */
typedef struct kas_rack_tables {
  kas_rack_impact*          racks;
  kas_scenario_rack_impact* scenarios;   /* [S] */
  int64_t*                  rack_off;    /* [S + 1], HOST memory in every entry point (may be NULL in the device form) */
  int64_t                   racks_cap;
} kas_rack_tables;

/* The rack impact of the plan's previous solve and impact pass: device_tables are the tables that solve used,
 * device_impact the records that impact pass wrote (device pointers; device_out->racks and ->scenarios too).
 * host_report_rack: HOST memory, node_pool_len entries, or NULL.  Asynchronous, ordered behind the plan's previous solve and
 * impact pass; it writes every record of its outputs itself.  A plan's first call, or a call whose table differs from the
 * previous call's (the contents are compared, not the pointer), uploads the plan's copy of the table and rack_off with
 * blocking copies; later calls only enqueue.
 * Refused before any GPU work, in this order: KAS_E_INVALID_ARG for a NULL argument or array, a non-NULL table for a batch
 * without nodes, or a negative entry of a scenario's table; KAS_E_UNSUPPORTED for a scenario with R_s > KAS_RACK_LIMIT;
 * KAS_E_INVALID_ARG for racks_cap below the sum of R_s; KAS_E_INVALID_ARG for a plan without a solve and an impact pass.
 * No scenario is refused for its node count: where the id lookup and the scenario's racks (uint16 per node) do not fit
 * the LDS together, the row kernel reads the racks from global memory. */
int kas_rack_impact_device(kas_plan* plan, const kas_tables* device_tables, const kas_impact_tables* device_impact,
                           const int32_t* host_report_rack, const kas_rack_tables* device_out, void* hip_stream);
int kas_rack_impact_device16(kas_plan* plan, const kas_tables16* device_tables, const kas_impact_tables* device_impact,
                             const int32_t* host_report_rack, const kas_rack_tables* device_out, void* hip_stream);

/* kas_solve_host_impact / 16 plus the rack pass on each scenario range's stream, right behind its impact pass; the rack
 * records, the scenario rack records and rack_off come back in host_racks (host memory).  host_impact->nodes may be NULL:
 * the node records then stay on the device — the call a rack report wants.  report_rack: as above (host memory).  The
 * refusals above apply, behind those of kas_solve_host_impact. */
int kas_solve_host_rack_impact(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables,
                               const int32_t* select, int32_t n_select, const kas_impact_tables* host_impact,
                               const int32_t* report_rack, const kas_rack_tables* host_racks);
int kas_solve_host16_rack_impact(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables,
                                 const int32_t* select, int32_t n_select, const kas_impact_tables* host_impact,
                                 const int32_t* report_rack, const kas_rack_tables* host_racks);

/* ---- ranking and fronting by rack criteria (added under ABI v6: purely additive) --------------------------------------
 * A *rack criterion* is a non-negative int32 taken from a scenario's kas_scenario_rack_impact.  Key KAS_KEY_RACK_BASE + i,
 * i = 0..14, is int32 word i of the record; two more are differences of its words.  kas_choose_spec and kas_front_spec take
 * these keys as they take the others (key[], limit_key[]), in any mix, but only in the *_racks entries below: every other
 * entry keeps refusing a key >= KAS_KEY_COUNT as an unknown criterion, and keys 10..15 are unknown everywhere. */
#define KAS_KEY_RACK_BASE                16
#define KAS_KEY_COLOCATED_BEFORE         16  /* kas_scenario_rack_impact.colocated_before                   */
#define KAS_KEY_COLOCATED_AFTER          17  /* .colocated_after                                            */
#define KAS_KEY_ROWS_COLOCATED_BEFORE    18  /* .rows_colocated_before                                      */
#define KAS_KEY_ROWS_COLOCATED_AFTER     19  /* .rows_colocated_after                                       */
#define KAS_KEY_SINGLE_RACK_ROWS_BEFORE  20  /* .single_rack_rows_before                                    */
#define KAS_KEY_SINGLE_RACK_ROWS_AFTER   21  /* .single_rack_rows_after                                     */
#define KAS_KEY_NEW_RACK_REPLICAS        22  /* .new_rack_replicas                                          */
#define KAS_KEY_ROWS_LOSING_RACKS        23  /* .rows_losing_racks                                          */
#define KAS_KEY_N_RACKS                  24  /* .n_racks                                                    */
#define KAS_KEY_MAX_RACK_INBOUND         25  /* .max_rack_inbound                                           */
#define KAS_KEY_MAX_RACK_OUTBOUND        26  /* .max_rack_outbound                                          */
#define KAS_KEY_MIN_RACK_REPLICAS_AFTER  27  /* .min_rack_replicas_after                                    */
#define KAS_KEY_MAX_RACK_REPLICAS_AFTER  28  /* .max_rack_replicas_after                                    */
#define KAS_KEY_MIN_RACK_LEADERS_AFTER   29  /* .min_rack_leaders_after                                     */
#define KAS_KEY_MAX_RACK_LEADERS_AFTER   30  /* .max_rack_leaders_after                                     */
#define KAS_KEY_RACK_REPLICA_SPREAD      31  /* max_rack_replicas_after - min_rack_replicas_after           */
#define KAS_KEY_RACK_LEADER_SPREAD       32  /* max_rack_leaders_after - min_rack_leaders_after             */
#define KAS_KEY_RACK_END                 33

/* Every entry below is its parent entry (the same name without _racks) with one more source of criteria, and orders, ties,
 * classes, offsets and determinism are the parent's.  A spec that names no rack criterion gives, with or without rack
 * records, the bytes the parent entry gives.  Refused with KAS_E_INVALID_ARG before any GPU work, in this order: the spec
 * refusals of the parent entry, with the same texts (a key is known when it is below KAS_KEY_COUNT or in KAS_KEY_RACK_BASE ..
 * KAS_KEY_RACK_END - 1); "rack criterion without rack records" when a key or a limit key is a rack criterion and the rack
 * records are NULL; then everything the parent entry refuses, in its order; then, in the host entries, the rack refusals of
 * kas_solve_host_rack_impact, in its order.  (ctx == NULL and n_scenarios < 0 are refused first, as in the parents.)
 *
 * kas_rank_device_racks / kas_front_rank_device_racks: kas_rank_device / kas_front_rank_device plus rack_scenarios[S], a
 * device array complete on the stream (NULL: no rack criterion may be named).  No plan. */
int kas_rank_device_racks(kas_ctx* ctx, const kas_scenario_result* scenario_results, const kas_scenario_impact* scenario_impact,
                          const kas_scenario_rack_impact* rack_scenarios, int32_t n_scenarios, const kas_choose_spec* spec,
                          int32_t* rank, int32_t* chosen, int32_t* n_ok, void* hip_stream);
int kas_front_rank_device_racks(kas_ctx* ctx, const kas_scenario_result* scenario_results, const kas_scenario_impact* scenario_impact,
                                const kas_scenario_rack_impact* rack_scenarios, int32_t n_scenarios, const kas_front_spec* spec,
                                int32_t* rank, int32_t* chosen, int32_t* counts, int32_t* scratch, void* hip_stream);

/* kas_choose_device / 16 and kas_front_device / 16 plus rack_scenarios: the DEVICE array of scenario rack records that the
 * plan's rack pass (kas_rack_impact_device / 16: device_out->scenarios) wrote for the plan's previous solve.  Ordered behind
 * that pass as behind the impact pass (the rack pass re-records the event a choice waits for); the gather is the parent's. */
int kas_choose_device_racks(kas_plan* plan, const kas_tables* device_tables, const kas_impact_tables* device_impact,
                            const kas_scenario_rack_impact* rack_scenarios, const kas_choose_spec* spec,
                            const kas_choice* device_choice, void* hip_stream);
int kas_choose_device16_racks(kas_plan* plan, const kas_tables16* device_tables, const kas_impact_tables* device_impact,
                              const kas_scenario_rack_impact* rack_scenarios, const kas_choose_spec* spec,
                              const kas_choice* device_choice, void* hip_stream);
int kas_front_device_racks(kas_plan* plan, const kas_tables* device_tables, const kas_impact_tables* device_impact,
                           const kas_scenario_rack_impact* rack_scenarios, const kas_front_spec* spec,
                           const kas_choice* device_choice, int32_t* counts, void* hip_stream);
int kas_front_device16_racks(kas_plan* plan, const kas_tables16* device_tables, const kas_impact_tables* device_impact,
                             const kas_scenario_rack_impact* rack_scenarios, const kas_front_spec* spec,
                             const kas_choice* device_choice, int32_t* counts, void* hip_stream);

/* kas_solve_host_choose_moves / 16 and kas_solve_host_front / 16 plus the rack pass of kas_solve_host_rack_impact on each
 * scenario range's stream, against report_rack (host memory, or NULL: the batch's node_rack); the ranking or the front waits
 * for every range's rack pass.  Rows, node blocks and moves come back for the chosen only; ALL rack records, scenario rack
 * records and rack_off come back in host_racks as from kas_solve_host_rack_impact (no rack blocks are gathered).
 * host_moves == NULL asks for no moves; host_choice->rows == NULL with rows_cap == 0 gathers no rows.  host_racks == NULL: no
 * rack pass and no rack records — the parent call, and no rack criterion may be named. */
int kas_solve_host_choose_racks(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables,
                                const kas_choose_spec* spec, const kas_choice* host_choice, const kas_impact_tables* host_impact,
                                const kas_moves* host_moves, const int32_t* report_rack, const kas_rack_tables* host_racks);
int kas_solve_host16_choose_racks(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables,
                                  const kas_choose_spec* spec, const kas_choice* host_choice, const kas_impact_tables* host_impact,
                                  const kas_moves* host_moves, const int32_t* report_rack, const kas_rack_tables* host_racks);
int kas_solve_host_front_racks(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables,
                               const kas_front_spec* spec, const kas_choice* host_choice, int32_t* counts,
                               const kas_impact_tables* host_impact, const kas_moves* host_moves, const int32_t* report_rack,
                               const kas_rack_tables* host_racks);
int kas_solve_host16_front_racks(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables,
                                 const kas_front_spec* spec, const kas_choice* host_choice, int32_t* counts,
                                 const kas_impact_tables* host_impact, const kas_moves* host_moves, const int32_t* report_rack,
                                 const kas_rack_tables* host_racks);

/* ---- topic impact: what a scenario does to each of its topics, reduced on the device (added under ABI v6) ---------------
 * A pass of its own behind a solve: nothing here depends on the impact pass having run.  Rows, C, O, clen, olen and "names a
 * node" are exactly those of kas_node_impact above.  The scenario-level spread hides what happens inside a topic (two topics
 * skewed in opposite directions sum to a flat cluster), and the reference bounds only a topic's maximum per broker, never the
 * minimum, and the leaders not at all.
 * Ranking or fronting by these figures is not part of this pass: the scenario record is laid out (sixteen non-negative int32)
 * so that its words are criteria of the *_topics entries below (KAS_KEY_TOPIC_BASE). */
#define KAS_TOPIC_SCRATCH_LIMIT (256ll << 20)   /* bytes of global counters one topic pass may need (see the refusals below) */

/* One per topic descriptor of the batch, in descriptor order: the fields of kas_scenario_impact, with the same meanings, taken
 * over THIS TOPIC'S rows only.  Max and min are over all nodes of the topic's scenario; a node that holds nothing of the topic
 * counts as 0.  Every field is 0 when the topic's status is not KAS_OK or the scenario has no nodes. */
typedef struct kas_topic_impact {
  int32_t departed_replicas;
  int32_t leaders_moved;
  int32_t max_inbound, max_outbound;              /* the most replicas of the topic one node receives / gives up */
  int32_t min_replicas_after, max_replicas_after;
  int32_t min_leaders_after, max_leaders_after;
} kas_topic_impact;

/* Per scenario, over its topics whose status is KAS_OK ("topics" below; a scenario without such topics gets zeros).  The
 * replica spread of a topic is max_replicas_after - min_replicas_after, its leader spread the same for leaders. */
typedef struct kas_scenario_topic_impact {
  int32_t topics_ok;                   /* word 0: number of KAS_OK topics                                   */
  int32_t topics_moved;                /*  1: topics with kas_topic_result.moved_replicas > 0               */
  int32_t topics_leaders_moved;        /*  2: topics with leaders_moved > 0                                 */
  int32_t topics_departed;             /*  3: topics with departed_replicas > 0                             */
  int32_t max_topic_moved_replicas;    /*  4: max over topics of kas_topic_result.moved_replicas            */
  int32_t max_topic_moved_partitions;  /*  5: ... of kas_topic_result.moved_partitions                      */
  int32_t max_topic_leaders_moved;     /*  6: max over topics of leaders_moved                              */
  int32_t max_topic_inbound;           /*  7: the most replicas of one topic that one node receives         */
  int32_t max_topic_outbound;          /*  8: the most replicas of one topic that one node gives up         */
  int32_t max_topic_replica_spread;    /*  9: max over topics of the replica spread                         */
  int32_t max_topic_leader_spread;     /* 10: ... of the leader spread                                      */
  int32_t max_topic_replicas_after;    /* 11: max over topics of max_replicas_after                         */
  int32_t max_topic_leaders_after;     /* 12: ... of max_leaders_after                                      */
  int32_t sum_topic_replica_spread;    /* 13: sum over topics of the replica spread                         */
  int32_t sum_topic_leader_spread;     /* 14: ... of the leader spread                                      */
  int32_t reserved;                    /* 15: 0                                                             */
} kas_scenario_topic_impact;

/* Where the records go: one kas_topic_impact per topic descriptor, one kas_scenario_topic_impact per scenario. */
typedef struct kas_topic_impact_tables {
  kas_topic_impact*          topics;      /* [n_topics]    */
  kas_scenario_topic_impact* scenarios;   /* [n_scenarios] */
} kas_topic_impact_tables;

/* The topic impact of the plan's previous solve: device_tables are the tables that solve used (device pointers;
 * device_out->topics and ->scenarios too).  Asynchronous, ordered behind the plan's previous solve (and its previous topic
 * pass); a later solve of the plan waits for it, as it waits for the impact pass.  It writes every record of its outputs
 * itself: nothing has to be cleared in front of the caller's arrays.  A plan's first call builds and uploads the pass's work
 * list with blocking copies; later calls only enqueue.
 * A topic whose scenario's n_nodes x 16 bytes of counters fit the LDS next to the id lookup (about 9,000 brokers) counts
 * there; a topic cut into row ranges (batches of few topics, as in the impact pass) adds its ranges' counters up in global
 * scratch, and a topic of a larger scenario counts in global scratch altogether: (4 n_nodes + 2) int32 per such topic.
 * Refused before any GPU work, in this order: KAS_E_INVALID_ARG for a NULL argument or array (device_out->topics with
 * n_topics > 0, ->scenarios with n_scenarios > 0, a table the pass reads); KAS_E_INVALID_ARG for a plan without a solve;
 * KAS_E_UNSUPPORTED when that global scratch would exceed KAS_TOPIC_SCRATCH_LIMIT bytes.  No scenario is refused for its
 * broker count up to KAS_N_LIMIT. */
int kas_topic_impact_device(kas_plan* plan, const kas_tables* device_tables, const kas_topic_impact_tables* device_out,
                            void* hip_stream);
int kas_topic_impact_device16(kas_plan* plan, const kas_tables16* device_tables, const kas_topic_impact_tables* device_out,
                              void* hip_stream);

/* kas_solve_host_impact / 16 plus the topic pass on each scenario range's stream, behind its solve; the records come back in
 * host_topics (host memory).  host_impact may be NULL: then no impact pass runs and no impact record is allocated or copied;
 * host_impact->nodes may be NULL as in kas_solve_host_rack_impact (the node records then stay on the device).
 * Refusals, behind those of kas_solve_host_impact and in the order above: KAS_E_INVALID_ARG for host_topics == NULL or an
 * array of it that is NULL; KAS_E_UNSUPPORTED for the scratch limit (taken over the whole batch). */
int kas_solve_host_topic_impact(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables,
                                const int32_t* select, int32_t n_select, const kas_impact_tables* host_impact,
                                const kas_topic_impact_tables* host_topics);
int kas_solve_host16_topic_impact(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables,
                                  const int32_t* select, int32_t n_select, const kas_impact_tables* host_impact,
                                  const kas_topic_impact_tables* host_topics);

/* ---- ranking and fronting by topic criteria (added under ABI v6: purely additive) -------------------------------------
 * A *topic criterion* is a non-negative int32 taken from a scenario's kas_scenario_topic_impact: key KAS_KEY_TOPIC_BASE + i,
 * i = 0..14, is int32 word i of the record (word 15, `reserved`, is no criterion, and there are no derived keys: the record
 * holds the spreads).  kas_choose_spec and kas_front_spec take these keys as they take the others (key[], limit_key[]), in
 * any mix with the broker and the rack criteria, but only in the *_topics entries below: the plain entries keep refusing a
 * key >= KAS_KEY_COUNT and the *_racks entries a key >= KAS_KEY_RACK_END as an unknown criterion, and keys 10..15 and 33..47
 * are unknown everywhere. */
#define KAS_KEY_TOPIC_BASE                  48
#define KAS_KEY_TOPICS_OK                   48  /* kas_scenario_topic_impact.topics_ok                       */
#define KAS_KEY_TOPICS_MOVED                49  /* .topics_moved                                             */
#define KAS_KEY_TOPICS_LEADERS_MOVED        50  /* .topics_leaders_moved                                     */
#define KAS_KEY_TOPICS_DEPARTED             51  /* .topics_departed                                          */
#define KAS_KEY_MAX_TOPIC_MOVED_REPLICAS    52  /* .max_topic_moved_replicas                                 */
#define KAS_KEY_MAX_TOPIC_MOVED_PARTITIONS  53  /* .max_topic_moved_partitions                               */
#define KAS_KEY_MAX_TOPIC_LEADERS_MOVED     54  /* .max_topic_leaders_moved                                  */
#define KAS_KEY_MAX_TOPIC_INBOUND           55  /* .max_topic_inbound                                        */
#define KAS_KEY_MAX_TOPIC_OUTBOUND          56  /* .max_topic_outbound                                       */
#define KAS_KEY_MAX_TOPIC_REPLICA_SPREAD    57  /* .max_topic_replica_spread                                 */
#define KAS_KEY_MAX_TOPIC_LEADER_SPREAD     58  /* .max_topic_leader_spread                                  */
#define KAS_KEY_MAX_TOPIC_REPLICAS_AFTER    59  /* .max_topic_replicas_after                                 */
#define KAS_KEY_MAX_TOPIC_LEADERS_AFTER     60  /* .max_topic_leaders_after                                  */
#define KAS_KEY_SUM_TOPIC_REPLICA_SPREAD    61  /* .sum_topic_replica_spread                                 */
#define KAS_KEY_SUM_TOPIC_LEADER_SPREAD     62  /* .sum_topic_leader_spread                                  */
#define KAS_KEY_TOPIC_END                   63

/* Every entry below is its *_racks parent (the same name with _racks for _topics) with one more source of criteria, and
 * orders, ties, classes, offsets and determinism are the parent's.  A spec that names no topic criterion gives, with or
 * without topic records, the bytes the *_racks entry gives.  Refused with KAS_E_INVALID_ARG before any GPU work, in this
 * order: the spec refusals of the parent entry, with the same texts (a key is known when it is below KAS_KEY_COUNT, in
 * KAS_KEY_RACK_BASE .. KAS_KEY_RACK_END - 1 or in KAS_KEY_TOPIC_BASE .. KAS_KEY_TOPIC_END - 1); "rack criterion without rack
 * records"; "topic criterion without topic records" when a key or a limit key is a topic criterion and the topic records are
 * NULL; then everything the *_racks entry refuses, in its order; then, in the host entries, the topic refusals of
 * kas_solve_host_topic_impact, in its order (KAS_E_UNSUPPORTED for the scratch limit among them).
 *
 * kas_rank_device_topics / kas_front_rank_device_topics: the *_racks entries plus topic_scenarios[S], a device array complete
 * on the stream.  Either of rack_scenarios and topic_scenarios may be NULL: no criterion of that set may then be named. */
int kas_rank_device_topics(kas_ctx* ctx, const kas_scenario_result* scenario_results, const kas_scenario_impact* scenario_impact,
                           const kas_scenario_rack_impact* rack_scenarios, const kas_scenario_topic_impact* topic_scenarios,
                           int32_t n_scenarios, const kas_choose_spec* spec, int32_t* rank, int32_t* chosen, int32_t* n_ok,
                           void* hip_stream);
int kas_front_rank_device_topics(kas_ctx* ctx, const kas_scenario_result* scenario_results, const kas_scenario_impact* scenario_impact,
                                 const kas_scenario_rack_impact* rack_scenarios, const kas_scenario_topic_impact* topic_scenarios,
                                 int32_t n_scenarios, const kas_front_spec* spec, int32_t* rank, int32_t* chosen, int32_t* counts,
                                 int32_t* scratch, void* hip_stream);

/* kas_choose_device_racks / 16 and kas_front_device_racks / 16 plus topic_scenarios: the DEVICE array of scenario topic
 * records that the plan's topic pass (kas_topic_impact_device / 16: device_out->scenarios) wrote for the plan's previous
 * solve.  A choice that names a topic criterion is ordered behind that pass (which records an event of its own) as well as
 * behind the impact pass, and a later topic pass or solve of the plan waits for the choice; the gather is the parent's. */
int kas_choose_device_topics(kas_plan* plan, const kas_tables* device_tables, const kas_impact_tables* device_impact,
                             const kas_scenario_rack_impact* rack_scenarios, const kas_scenario_topic_impact* topic_scenarios,
                             const kas_choose_spec* spec, const kas_choice* device_choice, void* hip_stream);
int kas_choose_device16_topics(kas_plan* plan, const kas_tables16* device_tables, const kas_impact_tables* device_impact,
                               const kas_scenario_rack_impact* rack_scenarios, const kas_scenario_topic_impact* topic_scenarios,
                               const kas_choose_spec* spec, const kas_choice* device_choice, void* hip_stream);
int kas_front_device_topics(kas_plan* plan, const kas_tables* device_tables, const kas_impact_tables* device_impact,
                            const kas_scenario_rack_impact* rack_scenarios, const kas_scenario_topic_impact* topic_scenarios,
                            const kas_front_spec* spec, const kas_choice* device_choice, int32_t* counts, void* hip_stream);
int kas_front_device16_topics(kas_plan* plan, const kas_tables16* device_tables, const kas_impact_tables* device_impact,
                              const kas_scenario_rack_impact* rack_scenarios, const kas_scenario_topic_impact* topic_scenarios,
                              const kas_front_spec* spec, const kas_choice* device_choice, int32_t* counts, void* hip_stream);

/* kas_solve_host_choose_racks / 16 and kas_solve_host_front_racks / 16 plus the topic pass of kas_solve_host_topic_impact on
 * each scenario range's stream, behind its solve; the ranking or the front waits for every range's passes.  ALL topic records
 * and scenario topic records come back in host_topics as from kas_solve_host_topic_impact.  host_topics == NULL: no topic
 * pass, and no topic criterion may be named; host_racks == NULL: no rack pass, and no rack criterion may be named.  The two
 * are independent. */
int kas_solve_host_choose_topics(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables,
                                 const kas_choose_spec* spec, const kas_choice* host_choice, const kas_impact_tables* host_impact,
                                 const kas_moves* host_moves, const int32_t* report_rack, const kas_rack_tables* host_racks,
                                 const kas_topic_impact_tables* host_topics);
int kas_solve_host16_choose_topics(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables,
                                   const kas_choose_spec* spec, const kas_choice* host_choice, const kas_impact_tables* host_impact,
                                   const kas_moves* host_moves, const int32_t* report_rack, const kas_rack_tables* host_racks,
                                   const kas_topic_impact_tables* host_topics);
int kas_solve_host_front_topics(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables,
                                const kas_front_spec* spec, const kas_choice* host_choice, int32_t* counts,
                                const kas_impact_tables* host_impact, const kas_moves* host_moves, const int32_t* report_rack,
                                const kas_rack_tables* host_racks, const kas_topic_impact_tables* host_topics);
int kas_solve_host16_front_topics(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables,
                                  const kas_front_spec* spec, const kas_choice* host_choice, int32_t* counts,
                                  const kas_impact_tables* host_impact, const kas_moves* host_moves, const int32_t* report_rack,
                                  const kas_rack_tables* host_racks, const kas_topic_impact_tables* host_topics);

/* ---- execution batches: a scenario's replica moves cut by per-broker caps, on the device (added under ABI v6: purely
 * additive) ------------------------------------------------------------------------------------------------------------
 * Nobody submits a move list of thousands of partitions to a live cluster as one reassignment: it is executed in batches,
 * with a limit on how many replicas a broker may be receiving at a time, how many it may be giving up, and how many
 * partitions a batch may hold.  Rows, C, O, clen, olen and "names a node" are exactly those of the kas_node_impact and
 * kas_move sections above; only topics whose kas_topic_result.status == KAS_OK contribute.
 * The *moves of a scenario* are its rows with the KAS_MOVE_REPLICAS flag, in (topic in descriptor order, row ascending)
 * order: the list kas_moves_device produces under mask == KAS_MOVE_REPLICAS; move i of that list is move i here.  For move i
 *   In(i)  = the set of nodes named by cells of O that are not in C,
 *   Out(i) = the set of nodes named by cells of C that are not in O (a cell of C that names no node of the scenario — a
 *            departed broker, KAS_CELL16_NONE — is in neither set: as kas_node_impact.outbound). */
typedef struct kas_batch_spec {      /* 0 = no bound; negative, or all three 0, or reserved != 0: KAS_E_INVALID_ARG */
  int32_t cap_inbound;               /* most moves of one batch that may have the same node in In()  */
  int32_t cap_outbound;              /* ... in Out()                                                   */
  int32_t max_moves;                 /* most moves in one batch                                        */
  int32_t reserved;
} kas_batch_spec;
/* Batches are consecutive ranges of the move list, defined by this loop:
 *   batch = empty; in[*] = out[*] = 0
 *   for i in moves, in order:
 *       why = MAX_MOVES if max_moves and batch.n_moves == max_moves
 *             else INBOUND  if cap_inbound  and any b in In(i)  has in[b]  == cap_inbound
 *             else OUTBOUND if cap_outbound and any b in Out(i) has out[b] == cap_outbound
 *             else none                         (tested in this order; the first that fails names the reason)
 *       if why: batch.closed_by = why; emit batch; batch = empty; in[*] = out[*] = 0
 *       add i to batch: in[b]++ for b in In(i); out[b]++ for b in Out(i)
 *   if batch not empty: batch.closed_by = END_OF_LIST; emit batch
 * A move adds at most 1 per node to each counter, so with caps >= 1 every batch holds a move and every batch is maximal. */
#define KAS_BATCH_END_OF_LIST 0
#define KAS_BATCH_MAX_MOVES   1
#define KAS_BATCH_INBOUND     2
#define KAS_BATCH_OUTBOUND    3
typedef struct kas_move_batch {      /* 32 bytes */
  int32_t first_move, n_moves;       /* moves [first_move, first_move + n_moves) of the scenario's REPLICAS move list */
  int32_t topic, partition;          /* of its first move, as kas_move.topic / .partition: a move list of ANY mask can be cut by these */
  int32_t replicas;                  /* sum of |In(i)| over its moves */
  int32_t max_inbound, max_outbound; /* max over nodes of the batch's counters */
  int32_t closed_by;                 /* KAS_BATCH_* */
} kas_move_batch;
typedef struct kas_scenario_batches {/* 32 bytes, eight non-negative int32; all 0 for an empty slot or a scenario without moves */
  int32_t n_batches;                 /* the TRUE count, whatever the room */
  int32_t n_moves, replicas;         /* over all batches */
  int32_t max_batch_moves, max_batch_replicas;
  int32_t closed_by_max_moves, closed_by_inbound, closed_by_outbound;   /* batches closed for that reason */
} kas_scenario_batches;
/* Where the records go (device pointers for kas_batches_device / 16, host pointers for the host forms).  A fixed stride per
 * listed scenario: the pass needs no second run and no scan between scenarios; a caller learns of truncation from
 * n_batches > stride, and records at or beyond min(n_batches, stride) are not touched.  A list entry of -1 is an empty slot;
 * a scenario may be listed twice (each listing gets a record and a block of its own); the same inputs give the same bytes. */
typedef struct kas_batches {
  kas_scenario_batches* scenarios;   /* [n]: one per LISTED scenario j */
  kas_move_batch* batches;           /* listed scenario j owns batches[j*stride .. j*stride + min(n_batches, stride)) */
  int64_t stride;                    /* >= 0; 0 with batches == NULL: the counts only */
} kas_batches;
/* A scenario's two counters per node live in the LDS next to the id lookup and the queue of moves: more nodes than this in
 * a LISTED scenario are KAS_E_UNSUPPORTED ((160 KiB - the queue of lists 8 wide - 288 bytes) / 12 bytes a node: kas_batches.h). */
#define KAS_BATCH_NODE_LIMIT 9362

/* The batches of the plan's previous solve, from the tables it used.  select: a DEVICE array of n_select scenario indices
 * (the chosen[] of a kas_choice is accepted as it is, with its -1 tail; an entry outside 0..S-1 is an empty slot).
 * Asynchronous; ordering, first-call allocation and the alignment refusals are those of kas_moves_device.
 * kas_batches_device16: the same for a plan of kas_plan_create16.
 * Refused before any GPU work, in this order: KAS_E_INVALID_ARG for the spec, a negative stride, a NULL array the call writes
 * (scenarios with n_select > 0; batches with stride > 0), misaligned pointers (records 4 bytes, cur / out to the cell
 * size); KAS_E_UNSUPPORTED for a plan with a scenario of more than KAS_BATCH_NODE_LIMIT nodes (the list is on the device:
 * every scenario of the plan counts), and for n_select x stride x 32 beyond 2^31 bytes. */
int kas_batches_device(kas_plan* plan, const kas_tables* device_tables, const int32_t* select, int32_t n_select,
                       const kas_batch_spec* spec, const kas_batches* device_out, void* hip_stream);
int kas_batches_device16(kas_plan* plan, const kas_tables16* device_tables, const int32_t* select, int32_t n_select,
                         const kas_batch_spec* spec, const kas_batches* device_out, void* hip_stream);

/* The host call that returns batches: the batch is solved, every topic record and scenario record comes back, no rows do
 * (host_tables->out may be NULL), plus the records of the scenarios in the HOST list select[0..n_select) (n_select < 0: every
 * scenario, in order).  The pass runs where the moves pass of kas_solve_host_moves runs: behind every scenario range.
 * Exactly the written records come back: n scenario records, and min(n_batches, stride) batch records per listed scenario.
 * Refused before any GPU work, in this order: what kas_solve_host_select refuses; the spec; a negative stride; a NULL array
 * the call writes; misaligned pointers (records 4 bytes); a list entry outside -1..S-1; KAS_E_UNSUPPORTED for a listed
 * scenario of more than KAS_BATCH_NODE_LIMIT nodes; KAS_E_UNSUPPORTED for n_select x stride x 32 beyond 2^31 bytes. */
int kas_solve_host_batches(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables, const int32_t* select,
                           int32_t n_select, const kas_batch_spec* spec, const kas_batches* host_out);
int kas_solve_host16_batches(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables, const int32_t* select,
                             int32_t n_select, const kas_batch_spec* spec, const kas_batches* host_out);

/* ---- packed rounds: a scenario's replica moves scheduled under per-broker caps, on the device (added under ABI v6: purely
 * additive) ------------------------------------------------------------------------------------------------------------
 * Partition reassignments are independent of each other, so nothing forces a cluster to execute a move list in list order.
 * A *round* is a set of moves executed together; the rounds pass gives every move of a scenario a round, so that in every
 * round no node is in In() of more than cap_inbound moves nor in Out() of more than cap_outbound, in far fewer rounds than
 * consecutive batches take.  Moves, In(i), Out(i), "names a node" and the contributing topics are exactly those of the
 * batches section above; the list is kas_moves_device's under mask == KAS_MOVE_REPLICAS, move i of that list is move i here.
 * (A bound on the moves of one round needs no scheduling: any round may be split into chunks without breaking a cap.) */
typedef struct kas_round_spec {      /* 0 = no bound on that direction; negative, or both caps 0, or policy != 0, or reserved != 0: KAS_E_INVALID_ARG */
  int32_t cap_inbound;               /* most moves of one round that may have the same node in In()  */
  int32_t cap_outbound;              /* ... in Out()                                                   */
  int32_t policy;                    /* KAS_ROUNDS_* */
  int32_t reserved;
} kas_round_spec;
#define KAS_ROUNDS_MONOTONE 0
/* Policy KAS_ROUNDS_MONOTONE — every node fills one round at a time and never returns to a round it left — is this loop:
 *   rin[*] = rout[*] = 0; uin[*] = uout[*] = 0          (the round a node is filling, the moves it holds there)
 *   for i in moves, in order:
 *       r = 0
 *       if cap_inbound:  for b in In(i):  r = max(r, uin[b]  < cap_inbound  ? rin[b]  : rin[b]  + 1)
 *       if cap_outbound: for b in Out(i): r = max(r, uout[b] < cap_outbound ? rout[b] : rout[b] + 1)
 *       round_of[i] = r
 *       if cap_inbound:  for b in In(i):  if rin[b]  == r: uin[b]++   else: rin[b]  = r; uin[b]  = 1
 *       if cap_outbound: for b in Out(i): if rout[b] == r: uout[b]++  else: rout[b] = r; uout[b] = 1
 *   n_rounds = 1 + max round_of, or 0 without moves
 * A (round, used) pair per node and direction suffices because a node never returns to a round it left; the price is room a true first
 * fit over all rounds would have used (DESIGN.md 10.9 has both against the lower bound ceil(max per-node total / cap)). */
typedef struct kas_move_round {      /* 16 bytes */
  int32_t n_moves;                   /* moves of the round (>= 1: every round below n_rounds holds a move) */
  int32_t replicas;                  /* sum of |In(i)| over them */
  int32_t first_move;                /* the lowest list index of a move of the round */
  int32_t reserved;                  /* 0 */
} kas_move_round;
typedef struct kas_scenario_rounds { /* 32 bytes, eight non-negative int32; all 0 for an empty slot or a scenario without moves */
  int32_t n_rounds;                  /* the TRUE count, whatever the room */
  int32_t n_moves, replicas;         /* over all rounds */
  int32_t max_round_moves, max_round_replicas;
  int32_t raised_by_inbound;         /* moves with r > 0 whose r an In node supplied */
  int32_t raised_by_outbound;        /* moves with r > 0 that only an Out node reached */
  int32_t reserved;                  /* 0 */
} kas_scenario_rounds;
/* Where the records go (device pointers for kas_rounds_device / 16, host pointers for the host forms).  Fixed strides per
 * listed scenario, for the reasons of kas_batches; a caller learns of truncation from n_rounds > round_stride or
 * n_moves > move_stride, and nothing at or beyond the written prefixes is touched.  Both strides 0: the counts only.  A list
 * entry of -1 is an empty slot; a scenario may be listed twice; the same inputs give the same bytes. */
typedef struct kas_rounds {
  kas_scenario_rounds* scenarios;    /* [n]: one per LISTED scenario j */
  kas_move_round* rounds;            /* listed j owns rounds[j*round_stride .. + min(n_rounds, round_stride)) */
  int64_t round_stride;              /* >= 0; 0 with rounds == NULL: none */
  int32_t* round_of;                 /* listed j owns round_of[j*move_stride .. + min(n_moves, move_stride)): the round of move i */
  int64_t move_stride;               /* >= 0; 0 with round_of == NULL: none */
} kas_rounds;
/* A scenario's (round, used) pair per node and direction lives in the LDS, packed into one 32-bit word, next to the id lookup,
 * the queue of moves and a window of round counters: more nodes than this in a LISTED scenario are KAS_E_UNSUPPORTED ((160 KiB -
 * the queue of lists 8 wide - the window - 288 bytes) / 12 bytes a node: kas_rounds.h).  The word gives the round the bits that
 * hold the scenario's row count P and `used` the rest: a cap above P never binds and is applied as no bound; any other cap of
 * 2^(32 - bits(P)) or more is KAS_E_UNSUPPORTED too (it takes a scenario of 65,536 rows or more and a cap of 32,768 or more). */
#define KAS_ROUND_NODE_LIMIT 9192

/* The rounds of the plan's previous solve, from the tables it used: the counterpart of kas_batches_device, with the same
 * list conventions (a DEVICE select[], a choice's chosen[] as it is), the same ordering (it waits for and re-records what a
 * moves pass does; a later solve waits for it) and the same refusals in the same order: KAS_E_INVALID_ARG for the spec, a
 * negative stride, a NULL array the call writes (scenarios with n_select > 0; rounds with round_stride > 0; round_of with
 * move_stride > 0), misaligned pointers; KAS_E_UNSUPPORTED for a plan with a scenario of more than KAS_ROUND_NODE_LIMIT nodes,
 * for a cap that does not fit a scenario's round words, and for n_select x round_stride x 16 or n_select x move_stride x 4 beyond 2^31 bytes. */
int kas_rounds_device(kas_plan* plan, const kas_tables* device_tables, const int32_t* select, int32_t n_select,
                      const kas_round_spec* spec, const kas_rounds* device_out, void* hip_stream);
int kas_rounds_device16(kas_plan* plan, const kas_tables16* device_tables, const int32_t* select, int32_t n_select,
                        const kas_round_spec* spec, const kas_rounds* device_out, void* hip_stream);

/* The host call that returns rounds: the counterpart of kas_solve_host_batches (no rows come back; a HOST list, n_select < 0:
 * every scenario; the pass runs behind every scenario range).  Exactly the written prefixes come back.  Refused before any GPU
 * work, in this order: what kas_solve_host_select refuses; the spec; a negative stride; a NULL array the call writes;
 * misaligned pointers (4 bytes); a list entry outside -1..S-1; KAS_E_UNSUPPORTED for a listed scenario of more than
 * KAS_ROUND_NODE_LIMIT nodes; KAS_E_UNSUPPORTED for a cap that does not fit a listed scenario's round words;
 * KAS_E_UNSUPPORTED for either stride's room. */
int kas_solve_host_rounds(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables* host_tables, const int32_t* select,
                          int32_t n_select, const kas_round_spec* spec, const kas_rounds* host_out);
int kas_solve_host16_rounds(kas_ctx* ctx, const kas_batch_desc* batch, const kas_tables16* host_tables, const int32_t* select,
                            int32_t n_select, const kas_round_spec* spec, const kas_rounds* host_out);

/* Pinned host memory for table pools (DMA without staging: see kas_solve_host).  A JNI caller wraps
 * it with NewDirectByteBuffer, a Python caller with numpy.frombuffer. */
int  kas_host_alloc(int64_t bytes, void** out_ptr);
void kas_host_free(void* ptr);

/* Sharding below Python (mirror of kafka-assigner_amd/sharding.py shard_range): scenarios
 * [*lo, *hi) of `total` belong to rank `rank` of `world` — contiguous, sizes differing by at most one,
 * the larger shards first. */
void kas_shard_range(int64_t total, int32_t rank, int32_t world, int64_t* lo, int64_t* hi);

/* Scenarios [lo, hi) of a batch as a batch of its own: `out` borrows the arrays of `b` (topic and node
 * pools narrowed to what the slice refers to) and uses scen_scratch[hi - lo] for the rebased scenario
 * descriptors; `tables_out` (optional, with `tables`) is the matching view of the result arrays — the
 * bulk pools stay whole, their offsets are absolute.  Topic descriptors of the slice's scenarios must
 * not be shared with scenarios outside it. */
int kas_batch_slice(const kas_batch_desc* b, int64_t lo, int64_t hi, kas_scenario_desc* scen_scratch,
                    kas_batch_desc* out, const kas_tables* tables, kas_tables* tables_out);

/* One batch over several devices: rank r of n_ctx solves kas_shard_range(S, r, n_ctx) on ctxs[r]
 * (one host thread per context, kas_solve_host on its slice), no communication — the scenarios are
 * independent and the caller's host arrays are the gather.  Contexts may sit on the same device.
 * A shard moves the whole extent of `out` / `ctx` its scenarios refer to, so the extents of consecutive
 * shards must not overlap (pools laid out in scenario order, the usual case); a batch whose extents do
 * overlap is solved on ctxs[0] alone — same results, no sharding. */
int kas_solve_host_sharded(kas_ctx* const* ctxs, int32_t n_ctx, const kas_batch_desc* batch,
                           const kas_tables* host_tables);

/* The hardware property the relaxation form of the preference ordering (lists <= 3 wide) and the fill kernel's quota draw
 * rest on — the LDS serves the lanes of one atomic-with-return instruction in ascending lane order; measured, not
 * documented — as this context's self-tests found it (kas_ctx_create, and again at every kas_plan_create of a batch
 * that may take the form, under LDS load on every CU and under partial EXEC masks): 1 held on every lane-operation
 * checked, 0 VIOLATED (the context uses the ticket forms and the draw without return from then on), -1 the test could
 * not run (same consequence), -2 switched off by the environment (KAS_NO_LANE_ORDER=1: the kill switch).
 * *lane_ops_checked (may be NULL): lane-operations checked so far.  See also KAS_PLAN_VERIFY_SAMPLE. */
int kas_ctx_lds_lane_order(const kas_ctx* ctx, int64_t* lane_ops_checked);

/* Counters of the host path since kas_ctx_create: calls, calls that found their plan in the
 * context's cache byte for byte, device allocations made (any pointer may be NULL). */
int kas_ctx_host_stats(kas_ctx* ctx, int64_t* calls, int64_t* plan_hits, int64_t* device_allocs);

/* Average device time in microseconds of one solve (both kernels) over the launches recorded since
 * the last call (HIP events on the launch stream); resets the accumulator. Returns <0 on
 * error, and *launches = 0 when nothing was recorded. */
int kas_plan_kernel_time_us(kas_plan* plan, double* avg_us, int* launches);

/* The same accumulator split in two: a solve is the fill kernel (P0-P3), first fit (P4: kas_p4_kernel behind the fill
 * where kas_plan_describe names it, inside the fill workgroup elsewhere) — together *fill_us — followed by the order
 * kernel (P5, *order_us) on one stream.  Either call resets the accumulator. */
int kas_plan_phase_times_us(kas_plan* plan, double* fill_us, double* order_us, int* launches);

/* Behaviour switches of a plan (default 0); every combination produces identical results, they
 * exist so that the alternative forms can be tested and timed on the same inputs.
 *   KAS_PLAN_GENERIC_FILL  always run the general multi-sweep sticky fill instead of the
 *                          rack-diverse histogram/quota form
 *   KAS_PLAN_ROUND_ORDER   always run the tile-round preference ordering instead of the relaxation / ticket forms
 *   KAS_PLAN_TICKET_ORDER  lists <= 3 wide: the ticket form of the preference ordering (three
 *                          wavefronts per pair of scenarios) where the relaxation form (one wavefront per scenario,
 *                          kas_order_relax.h) would run; KAS_PLAN_WIDE_COUNTERS and KAS_PLAN_GROUPS(n != 0), which
 *                          only mean something to the ticket form, imply it
 *   KAS_PLAN_WIDE_COUNTERS ticket form with 4 x uint16 counter rows even where three 10-bit counts
 *                          in one uint32 would do
 *   KAS_PLAN_TWO_PASS_HIST rack-diverse fill with one histogram for the whole topic and a separate
 *                          chunk-count pass over cur, instead of per-chunk histograms
 *   KAS_PLAN_SPREAD_FILL   take the spread fill (the row scans of large single-topic scenarios over many
 *                          one-wavefront workgroups; chosen by itself for batches of <= 64 scenarios
 *                          of >= 131,072 partitions) for any single-topic batch, with few chunks
 *   KAS_PLAN_RELAX_TILES(n) relaxation form: 1 = tiles of 64 rows, 2 = double tiles (128 rows, two rows per lane: fewer
 *                          LDS round trips per scenario, more LDS operations per row), 0 = by batch size (double
 *                          tiles for batches of fewer than 512 scenarios, where the GPU is not full of wavefronts).
 *                          Lists 4 and 5 wide (round 6): 1 = the relaxation form for these widths (kas_order_relax_wide.h: one
 *                          wavefront per scenario, uint64 counter words; batches without a Context) instead of the wide ticket
 *                          form — exact, and measured slower at BASELINE configs[4], hence opt-in
 *                          3 (round 6) = quad tiles: 256 rows a step, four rows per lane — instances exist on dword mid rows only
 *                          (elsewhere: double tiles); exact, and measured SLOWER than double tiles for a batch alone (order kernel
 *                          1.54 against 1.42 ms per 1000 scenarios), hence only on request
 *   KAS_PLAN_INDEX_ROWS / KAS_PLAN_NO_INDEX_ROWS  rack-diverse fill with per-chunk histograms on int32 cells (round 6): with index
 *                          rows the first row scan — which looks every broker id up, KAS:118-119's nodeMap.get — leaves the row's
 *                          node indices where its mid row goes, the second scan streams those 2-byte cells and stores only the rows
 *                          that do not keep all their replicas: `cur` is read ONCE and every id is looked up once; without, `cur` is
 *                          read by both scans.  Neither flag: the library's default (DESIGN.md section 4.1 has the measurement).
 *   KAS_PLAN_MID32 / KAS_PLAN_NO_MID32  dword mid rows (round 6): between the fill and the order kernel a row of up to three holders
 *                          is ONE aligned dword — the holders sorted by node index, 11 bits each (nothing behind the fill depends on
 *                          their order: first fit appends, KAS:228 sorts) — instead of three uint16 in acceptance order: 4 instead
 *                          of 6 bytes a row written and read, one memory instruction where the packed row takes two, and the order
 *                          kernel's tags become the topic's constants.  Applies to int32 cells, lists 3 wide, at most 2,047 brokers,
 *                          the relaxation form without a Context or sampled verification; otherwise (and with KAS_PLAN_INDEX_ROWS) the
 *                          16-bit rows.  Neither flag: the library's default (DESIGN.md section 4.6 has the measurement).
 *   KAS_PLAN_FULL_FILL     kas_fill_kernel for every scenario.  Default (round 6; int32 cells, lists up to 3 wide, per-chunk
 *                          histograms, a direct id table, first fit handed over): kas_fill_slim_kernel first — the one path
 *                          rack-diverse scenarios take, compiled without the others (120 VGPRs, no scratch) — and
 *                          kas_fill_kernel behind it, on a small grid, for the scenarios it hands back (rows not rack-diverse, ...)
 *   KAS_PLAN_NO_RTN_QUOTA  rack-diverse fill with per-chunk histograms: draw a node's quota with separate LDS atomics,
 *                          reads and a ranking of the tiles in which it runs out, instead of one atomic-with-return
 *                          per list position
 *   KAS_PLAN_FILL_WITH_P4 / KAS_PLAN_SPLIT_P4  first fit (KAS:162-186) inside the fill kernel's workgroup (four wavefronts
 *                          hand the windows over through LDS) / in kas_p4_kernel behind it (one wavefront per scenario),
 *                          whatever the batch size.  Default: kas_p4_kernel for batches of >= 512 scenarios — it
 *                          frees the fill workgroup's registers and LDS early, which is what counts when several
 *                          batches share the GPU — and inside the fill workgroup below that and in kas_solve_host's
 *                          plans (a batch alone on the GPU: the shorter critical path counts).
 *   KAS_PLAN_P4_WITH_ORDER (= both of the above; round 6)  first fit as a second wavefront of the ORDER kernel's workgroup
 *                          (kas_p4_order_kernel; lists up to 3 wide on the relaxation form, no Context, no sampled verification —
 *                          otherwise kas_p4_kernel): the order wavefront follows first fit's progress row by row instead of
 *                          waiting behind a kernel boundary, so a batch that has the GPU to itself lasts
 *                          fill + max(first fit, order) instead of fill + first fit + order
 *   KAS_PLAN_VERIFY_SAMPLE(k) relaxation form: k tiles of 64 rows per topic (evenly spaced, 1..255) are evaluated a second
 *                          time one row at a time — independent of how the LDS orders the lanes of an instruction —
 *                          and a scenario in which a row comes out differently reports KAS_FAIL_WATCHDOG instead of a
 *                          list (an opt-in canary for production: ~3 us per verified tile; the kernel always checks
 *                          that the counters it leaves sum to the rows it retired)
 *   KAS_PLAN_WAVES(n)      wavefronts per scenario workgroup of the fill kernel: 1, 2 or 4
 *   KAS_PLAN_GROUPS(n)     scenarios per wavefront of the ticket-form order kernel: 1, 2 or 4
 *                          (0 = the plan's choice for either) */
#define KAS_PLAN_GENERIC_FILL 1u
#define KAS_PLAN_ROUND_ORDER  2u
#define KAS_PLAN_WIDE_COUNTERS 4u
#define KAS_PLAN_TWO_PASS_HIST 8u
#define KAS_PLAN_FULL_FILL    16u
#define KAS_PLAN_SPREAD_FILL  32u
#define KAS_PLAN_NO_INDEX_ROWS 64u
#define KAS_PLAN_INDEX_ROWS  128u
#define KAS_PLAN_MID32        0x80000u
#define KAS_PLAN_NO_MID32     0x100000u
#define KAS_PLAN_TICKET_ORDER 0x10000u
#define KAS_PLAN_RELAX_TILES(n) (((uint32_t)(n) & 3u) << 17)
#define KAS_PLAN_NO_RTN_QUOTA 0x200000u
#define KAS_PLAN_SPLIT_P4     0x400000u
#define KAS_PLAN_FILL_WITH_P4 0x800000u
#define KAS_PLAN_VERIFY_SAMPLE(k) (((uint32_t)(k) & 0xffu) << 24)
#define KAS_PLAN_WAVES(n)     (((uint32_t)(n) & 0xfu) << 8)
#define KAS_PLAN_GROUPS(n)    (((uint32_t)(n) & 0xfu) << 12)
int kas_plan_set_flags(kas_plan* plan, uint32_t flags);

/* Per-scenario device counters of the plan's most recent solve (after it completed), 16 int64
 * per scenario; times in 10 ns ticks of the constant 100 MHz device clock:
 *   [0] setup  [1] P2 histogram + quota  [2] P2 keep-scan + P3  [3] P4 first fit
 *   [4] P4 windows  [5] P4 node steps  [6] P5 rounds (round form)
 *   [7] P2 tiles of wave 0 that needed quota ranking  [8] order kernel time
 *   ([4], [5], [7], [15] are zero unless the library was built with -DKAS_FILL_COUNTERS)
 *   ticket form: [9] solver steps  [11] of those with rows in hand but none ready
 *                [6] steps that took the queue path  [10] wins / prefix-sum rounds spent there
 *                [14] rows decided inside queues  [15] sum over steps of rows in hand
 *                [12] stager iterations  [13] of those without work
 *   wide ticket form (lists 4, 5 wide): [9]..[11], [6], [14] are the class-1 solver's, [15] = steps of
 *                the first class-0 solver
 *   ([4], [5] count wave 0's share of the P4 windows / node positions)
 * n = capacity of out in int64 elements (>= KAS_STATS_PER_SCENARIO * n_scenarios).  Blocks until the
 * plan's last launch has finished. */
#define KAS_STATS_PER_SCENARIO 16
int kas_plan_stats(kas_plan* plan, int64_t* out, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* KAS_ABI_H */
