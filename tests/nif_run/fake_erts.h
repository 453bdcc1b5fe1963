/*
 * tests/nif_run/fake_erts.h -- TEST INFRASTRUCTURE ONLY: what the driver
 * (beam_main.c) needs from the stand-in erl_nif runtime (fake_erts.c) beyond
 * the enif_* prototypes of tests/nif_lint/erl_nif.h.
 */
#ifndef PSIM_FAKE_ERTS_H
#define PSIM_FAKE_ERTS_H
#include <erl_nif.h>
#include <stdio.h>

struct enif_environment_t { int exception; };

/* term construction for the script parser (the shim's own come from enif_make_*) */
ERL_NIF_TERM fe_make_script_binary(const unsigned char *bytes, size_t size, int aligned);
ERL_NIF_TERM fe_make_tuple(const ERL_NIF_TERM *e, unsigned n);
/* 0 when the key is already there */
int fe_map_put(ERL_NIF_TERM map, ERL_NIF_TERM key, ERL_NIF_TERM value, ERL_NIF_TERM *out);
/* {ok, X} -> 1 and *x = X */
int fe_ok_payload(ERL_NIF_TERM t, ERL_NIF_TERM *x);
void fe_print(FILE *f, ERL_NIF_TERM t);

/* the term arena is a stack: everything made after fe_mark() goes at fe_release(mark) */
size_t fe_mark(void);
void fe_release(size_t mark);

/* failure injection: the k-th call from now fails (k = 1: the next) */
enum { FE_ALLOC, FE_ALLOC_BINARY, FE_ALLOC_RESOURCE, FE_MUTEX_CREATE, FE_NFAIL };
void fe_fail(int what, unsigned k);
void fe_busy_next_trylock(void);

/* accounting */
typedef struct { long allocs, binaries, resources, mutexes, held_by_me; } fe_live_t;
fe_live_t fe_live(void);
/* lists what is still alive on f; the number of items */
long fe_report_leaks(FILE *f);
#endif
