/* exchange.c — the ONE exchange that ends the stream of a multi-rank job (multi.c): every rank's partial, summed onto rank 0
 * (RCCL over xGMI, or files when some rank has no communicator), and the communicator made beside the scan. */
#define _GNU_SOURCE
#include "itx_host.h"

#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

/* The communicator of a multi-rank job is made while the stream is being read: ncclCommInitRank takes seconds (bootstrap
 * over the network interface, one ring per link) and needs nothing of the data — the exchange at the end only joins it. */
static struct {
    pthread_t th;
    int on, rc, done;
    itx_comm *comm;
    char err[400];
} early_comm;
/* Which way the partials travel is agreed on by ALL ranks: every rank leaves a marker next to the communicator id when its
 * attempt at an RCCL communicator has ended — "ok" or "fail" — and the exchange is RCCL only when every marker says ok. A
 * rank that fails alone (its device, its copy of the library, the id file) would otherwise switch to files while the others
 * sit in ncclCommInitRank / ncclReduce, which have no timeout. */
static void comm_marker_path(char *buf, size_t n, int rank) { snprintf(buf, n, "%s.st%d", multi_comm_id(), rank); }
static void comm_marker_write(int ok)
{
    if (multi_world() <= 1) return;
    char path[700], tmp[720];
    comm_marker_path(path, sizeof path, multi_rank());
    snprintf(tmp, sizeof tmp, "%s.tmp", path);
    FILE *f = fopen(tmp, "w");
    if (!f) return;
    fputs(ok ? "ok" : "fail", f);
    if (fclose(f) == 0 && rename(tmp, path) != 0) unlink(tmp);
}
/* 1: every rank has a communicator; 0: some rank has none (all take the files); -1: a marker never came */
static int comm_agree(double timeout_s)
{
    const double t0 = now_s();
    for (unsigned spins = 0;; spins++) {
        int n_ok = 0;
        for (int r = 0; r < multi_world(); r++) {
            char path[700], w[8] = {0};
            comm_marker_path(path, sizeof path, r);
            FILE *f = fopen(path, "r");
            if (!f) continue;
            const size_t k = fread(w, 1, 7, f);
            fclose(f);
            if (k >= 4 && memcmp(w, "fail", 4) == 0) return 0;
            if (k >= 2 && memcmp(w, "ok", 2) == 0) n_ok++;
        }
        if (n_ok == multi_world()) return 1;
        if (now_s() - t0 > timeout_s) return -1;
        usleep(spins < 2000 ? 200 : 2000);
    }
}
static void comm_markers_remove(void)
{
    for (int r = 0; r < multi_world(); r++) {
        char path[700];
        comm_marker_path(path, sizeof path, r);
        unlink(path);
    }
}
static void *early_comm_main(void *arg)
{
    (void)arg;
    early_comm.rc = itx_comm_create(multi_rank(), multi_world(), multi_device(), multi_comm_id(), ITX_COMM_RCCL, &early_comm.comm);
    if (early_comm.rc != ITX_OK) snprintf(early_comm.err, sizeof early_comm.err, "%s", itx_last_error());
    comm_marker_write(early_comm.rc == ITX_OK);
    __atomic_store_n(&early_comm.done, 1, __ATOMIC_RELEASE);
    return NULL;
}

int exchange_comm_early_wanted(void)
{
    return (multi_world() > 1 || multi_selftest()) && multi_comm_mode() == ITX_COMM_RCCL && !getenv("ITX_NO_EARLY_COMM");
}

void exchange_comm_early(void)
{
    if (exchange_comm_early_wanted() && pthread_create(&early_comm.th, NULL, early_comm_main, NULL) == 0) early_comm.on = 1;
}

/* the RCCL communicator the early thread made, when every rank has one; else the files, agreed on through the markers */
static itx_comm *join_comm(int *comm_mode)
{
    const int rank = multi_rank(), world = multi_world();
    itx_comm *comm = NULL;
    int crc = ITX_OK;
    if (*comm_mode != ITX_COMM_RCCL) {
        chk(itx_comm_create(rank, world, multi_device(), multi_comm_id(), *comm_mode, &comm), "itx_comm_create");
        return comm;
    }
    if (!early_comm.on) {                                    /* not under way since the start of the run: make it now, same thread function */
        if (pthread_create(&early_comm.th, NULL, early_comm_main, NULL) == 0) {
            early_comm.on = 1;
        } else {
            early_comm.rc = ITX_E_STATE;
            snprintf(early_comm.err, sizeof early_comm.err, "no thread for the communicator");
            comm_marker_write(0);
            early_comm.done = 1;
        }
    }
    const char *te = getenv("ITX_COMM_TIMEOUT");
    int agreed;
    if (world > 1) {
        agreed = comm_agree(te && atof(te) > 0 ? atof(te) : 900.0);
    } else {                                                 /* ITX_COMM_SELFTEST: a job of one rank agrees with itself */
        if (early_comm.on) pthread_join(early_comm.th, NULL);
        early_comm.on = 0;
        agreed = early_comm.rc == ITX_OK;
    }
    if (agreed < 0) die("rank %d: the other ranks never said whether they have a communicator (a rank of the job has died?)", rank);
    if (agreed == 1 || __atomic_load_n(&early_comm.done, __ATOMIC_ACQUIRE)) {
        if (early_comm.on) pthread_join(early_comm.th, NULL);
        early_comm.on = 0;
        crc = early_comm.rc;
        comm = early_comm.comm;
    } else {
        early_comm.on = 0;                                   /* still inside ncclCommInitRank, waiting for a rank that will not come: left behind */
        crc = ITX_E_STATE;
    }
    if (agreed == 0) {
        /* some rank has no RCCL communicator (no usable network interface for its bootstrap, its device, its library):
         * every rank has seen the same markers and hands its partial over through files — slower, same sums */
        if (early_comm.err[0]) warnf("[iteres] note: no RCCL communicator (%s); the ranks exchange through files instead", early_comm.err);
        else warnf("[iteres] note: another rank has no RCCL communicator; the ranks exchange through files instead");
        if (crc == ITX_OK && comm) itx_comm_destroy(comm);
        comm = NULL;
        *comm_mode = ITX_COMM_FILE;
        crc = itx_comm_create(rank, world, multi_device(), multi_comm_id(), *comm_mode, &comm);
    }
    chk(crc, "itx_comm_create");
    return comm;
}

void exchange_partials(itx_engine *eng, uint64_t *meta, size_t n_meta, int timing, void **p64, void **p32)
{
    const int rank = multi_rank(), world = multi_world();
    const double tx = now_s();
    uint64_t n64 = 0, n32 = 0;
    chk(itx_engine_partial_buffers(eng, p64, p32), "itx_engine_partial_buffers");
    chk(itx_engine_partial_size(eng, &n64, &n32), "itx_engine_partial_size");
    chk(itx_engine_sync(eng), "itx_engine_sync");
    chk(itx_engine_export_partial(eng, *p64, *p32, NULL), "itx_engine_export_partial");
    const double tc = now_s();
    int comm_mode = multi_comm_mode();
    itx_comm *comm = join_comm(&comm_mode);
    const double ty = now_s();
    chk(itx_comm_reduce_sum(comm, *p64, n64, *p32, n32, meta, n_meta, NULL), "itx_comm_reduce_sum");
    if (timing && rank == 0)
        fprintf(stderr, "[itx timing] exchange (%s): export %.3f s, communicator %.3f s, reduce of %.1f MB per rank (waits for the slowest rank) %.3f s\n",
                comm_mode == ITX_COMM_FILE ? "files" : "RCCL", tc - tx, ty - tc, (double)(n64 * 8 + n32 * 4) / 1e6, now_s() - ty);
    itx_comm_destroy(comm);
    if (rank == 0 && world > 1) {
        comm_markers_remove();                                   /* every rank has read them: its partial is here */
        /* RCCL was given up for the files: the communicator id this rank may have written for it (its thread still sits in
         * ncclCommInitRank, waiting for a rank that will not come) goes too */
        if (comm_mode == ITX_COMM_FILE && multi_comm_mode() == ITX_COMM_RCCL) unlink(multi_comm_id());
    }
    if (rank > 0) {                                              /* handed over: rank 0 writes the files */
        fflush(NULL);
        _exit(0);
    }
}
