/*
 * tests/nif_run/fake_erts.c -- TEST INFRASTRUCTURE ONLY: a stand-in for the
 * part of the erl_nif runtime that erlang/c_src/partisan_gpu_sim_nif.c uses,
 * so that the shim can execute in an image without Erlang.  Written from the
 * published erl_nif documentation, over the prototypes of
 * tests/nif_lint/erl_nif.h.  Where the documentation leaves behaviour
 * undefined this runtime is stricter than the BEAM: it aborts with a message
 * on a second release of a binary, an unlock by a thread that does not hold
 * the mutex, an atom name over 255 bytes, a term that is none.
 *
 * Terms live in one arena used as a stack (fe_mark / fe_release); a term is
 * its arena index plus TERM_BASE.  One lock guards every registry; an
 * ErlNifMutex is a pthread mutex of its own.
 */
#include "fake_erts.h"

#include <errno.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define TERM_BASE 0x7E0000000000ul
#define CHUNK 65536u
#define NCHUNKS 16384u

enum { T_INT, T_ATOM, T_TUPLE, T_NIL, T_CONS, T_MAP, T_BIN, T_RES };
typedef struct {
    uint8_t kind;
    uint32_t n;          /* tuple arity, map pairs, binary size (low bits in u too) */
    uint64_t u;          /* integer value, atom index, binary size */
    void *p;             /* elements (tuple n, cons 2, map 2n), binary data, resource object */
    void *base;          /* binary: the allocation a term owns (NULL: a made binary's record) */
} term;

static pthread_mutex_t G = PTHREAD_MUTEX_INITIALIZER;
static term *chunks[NCHUNKS];
static size_t top;

static void die(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fputs("fake_erts: ", stderr);
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
    va_end(ap);
    fflush(NULL);
    abort();
}

static void *xmalloc(size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p) die("host malloc failed");
    return p;
}

static term *T(ERL_NIF_TERM t) {
    size_t i = (size_t)(t - TERM_BASE);
    if (t < TERM_BASE || i >= top) die("not a term: %#lx", t);
    return &chunks[i / CHUNK][i % CHUNK];
}

static ERL_NIF_TERM new_term(term v) {
    pthread_mutex_lock(&G);
    size_t i = top;
    if (i / CHUNK >= NCHUNKS) die("term arena full");
    if (!chunks[i / CHUNK]) chunks[i / CHUNK] = xmalloc(CHUNK * sizeof(term));
    chunks[i / CHUNK][i % CHUNK] = v;
    top = i + 1;
    pthread_mutex_unlock(&G);
    return TERM_BASE + i;
}

/* ------------------------------------------------------------ injection -- */
static unsigned fail_at[FE_NFAIL];
static int busy_next;

void fe_fail(int what, unsigned k) { fail_at[what] = k; }
void fe_busy_next_trylock(void) { busy_next = 1; }

static int inject(int what) {
    int hit = 0;
    pthread_mutex_lock(&G);
    if (fail_at[what] && --fail_at[what] == 0) hit = 1;
    pthread_mutex_unlock(&G);
    return hit;
}

/* --------------------------------------------------------- enif_alloc -- */
#define A_LIVE 0xA110C8EDu
#define A_FREED 0xDEADF4EEu
typedef struct ahdr { uint32_t magic; size_t size; struct ahdr *prev, *next; long serial; uint64_t pad; } ahdr;
static ahdr *allocs;
static long n_allocs, alloc_serial;

void *enif_alloc(size_t size) {
    if (inject(FE_ALLOC)) return NULL;
    ahdr *a = xmalloc(sizeof *a + size);
    pthread_mutex_lock(&G);
    a->magic = A_LIVE; a->size = size; a->prev = NULL; a->next = allocs; a->serial = ++alloc_serial;
    if (allocs) allocs->prev = a;
    allocs = a;
    n_allocs++;
    pthread_mutex_unlock(&G);
    return a + 1;
}

void enif_free(void *ptr) {
    if (!ptr) die("enif_free(NULL)");
    ahdr *a = (ahdr *)ptr - 1;
    pthread_mutex_lock(&G);
    if (a->magic != A_LIVE) die("enif_free of a block that is not live (%s)", a->magic == A_FREED ? "freed twice" : "foreign");
    a->magic = A_FREED;
    if (a->prev) a->prev->next = a->next; else allocs = a->next;
    if (a->next) a->next->prev = a->prev;
    n_allocs--;
    pthread_mutex_unlock(&G);
    free(a);
}

/* ------------------------------------------------------------ binaries -- */
enum { B_OWNED = 1, B_MADE, B_RELEASED };
typedef struct brec { int state; unsigned char *data; size_t size; struct brec *next; long serial; } brec;
static brec *brecs;
static long n_owned, bin_serial;

int enif_alloc_binary(size_t size, ErlNifBinary *bin) {
    if (inject(FE_ALLOC_BINARY)) return 0;
    brec *b = xmalloc(sizeof *b);
    b->state = B_OWNED; b->size = size; b->data = xmalloc(size);
    memset(b->data, 0xA5, size);
    pthread_mutex_lock(&G);
    b->next = brecs; brecs = b; b->serial = ++bin_serial;
    n_owned++;
    pthread_mutex_unlock(&G);
    bin->size = size; bin->data = b->data; bin->ref_bin = b;
    return 1;
}

static brec *owned(ErlNifBinary *bin, const char *who) {
    brec *b = (brec *)bin->ref_bin;
    if (!b) die("%s of a binary that enif_alloc_binary did not make", who);
    if (b->state != B_OWNED)
        die("%s of a binary already %s", who, b->state == B_MADE ? "made into a term" : "released");
    return b;
}

void enif_release_binary(ErlNifBinary *bin) {
    pthread_mutex_lock(&G);
    brec *b = owned(bin, "enif_release_binary");
    b->state = B_RELEASED;
    n_owned--;
    pthread_mutex_unlock(&G);
    free(b->data);
    b->data = NULL;
}

ERL_NIF_TERM enif_make_binary(ErlNifEnv *env, ErlNifBinary *bin) {
    pthread_mutex_lock(&G);
    brec *b = owned(bin, "enif_make_binary");
    b->state = B_MADE;
    n_owned--;
    pthread_mutex_unlock(&G);
    term v = {T_BIN, 0, b->size, b->data, b->data};
    b->data = NULL;
    return new_term(v);
}

ERL_NIF_TERM fe_make_script_binary(const unsigned char *bytes, size_t size, int aligned) {
    /* malloc's result is 16-byte aligned: one byte in, the data sits at an odd
     * address, and the allocation ends with the data either way */
    unsigned char *base = xmalloc(size + (aligned ? 0 : 1));
    unsigned char *data = base + (aligned ? 0 : 1);
    if (size) memcpy(data, bytes, size);
    term v = {T_BIN, 0, size, data, base};
    return new_term(v);
}

int enif_inspect_binary(ErlNifEnv *env, ERL_NIF_TERM t, ErlNifBinary *bin) {
    term *x = T(t);
    if (x->kind != T_BIN) return 0;
    bin->size = (size_t)x->u; bin->data = x->p; bin->ref_bin = NULL;
    return 1;
}

/* ----------------------------------------------------------- resources -- */
struct enif_resource_type_t { char name[64]; ErlNifResourceDtor *dtor; };
#define R_LIVE 0x4E50114Eu
typedef struct rhdr { uint32_t magic; long refc; ErlNifResourceType *type; size_t size; struct rhdr *prev, *next; long serial; uint64_t pad; } rhdr;
static rhdr *resources;
static long n_resources, res_serial;

ErlNifResourceType *enif_open_resource_type(ErlNifEnv *env, const char *module_str, const char *name_str,
                                            ErlNifResourceDtor *dtor, ErlNifResourceFlags flags,
                                            ErlNifResourceFlags *tried) {
    if (module_str) die("enif_open_resource_type: module_str must be NULL");
    if (!(flags & ERL_NIF_RT_CREATE)) return NULL;
    ErlNifResourceType *t = xmalloc(sizeof *t);
    snprintf(t->name, sizeof t->name, "%s", name_str);
    t->dtor = dtor;
    if (tried) *tried = ERL_NIF_RT_CREATE;
    return t;          /* (lives as long as the program, as a loaded module's does) */
}

void *enif_alloc_resource(ErlNifResourceType *type, size_t size) {
    if (!type) die("enif_alloc_resource: no type");
    if (inject(FE_ALLOC_RESOURCE)) return NULL;
    rhdr *r = xmalloc(sizeof *r + size);
    memset(r + 1, 0xA5, size);
    pthread_mutex_lock(&G);
    r->magic = R_LIVE; r->refc = 1; r->type = type; r->size = size; r->serial = ++res_serial;
    r->prev = NULL; r->next = resources;
    if (resources) resources->prev = r;
    resources = r;
    n_resources++;
    pthread_mutex_unlock(&G);
    return r + 1;
}

static rhdr *res_hdr(void *obj, const char *who) {
    rhdr *r = (rhdr *)obj - 1;
    if (!obj || r->magic != R_LIVE) die("%s: not a live resource", who);
    return r;
}

void enif_release_resource(void *obj) {
    pthread_mutex_lock(&G);
    rhdr *r = res_hdr(obj, "enif_release_resource");
    long left = --r->refc;
    if (left == 0) {
        if (r->prev) r->prev->next = r->next; else resources = r->next;
        if (r->next) r->next->prev = r->prev;
        n_resources--;
    }
    pthread_mutex_unlock(&G);
    if (left < 0) die("enif_release_resource: reference count below zero");
    if (left == 0) {
        if (r->type->dtor) r->type->dtor(NULL, obj);
        r->magic = 0;
        free(r);
    }
}

ERL_NIF_TERM enif_make_resource(ErlNifEnv *env, void *obj) {
    pthread_mutex_lock(&G);
    res_hdr(obj, "enif_make_resource")->refc++;
    pthread_mutex_unlock(&G);
    term v = {T_RES, 0, 0, obj, NULL};
    return new_term(v);
}

int enif_get_resource(ErlNifEnv *env, ERL_NIF_TERM t, ErlNifResourceType *type, void **objp) {
    term *x = T(t);
    if (x->kind != T_RES || res_hdr(x->p, "enif_get_resource")->type != type) return 0;
    *objp = x->p;
    return 1;
}

/* ------------------------------------------------------------- mutexes -- */
struct enif_mutex_t { pthread_mutex_t m; int held; pthread_t owner; char name[32]; struct enif_mutex_t *prev, *next; };
static ErlNifMutex *mutexes;
static long n_mutexes;

ErlNifMutex *enif_mutex_create(char *name) {
    if (inject(FE_MUTEX_CREATE)) return NULL;
    ErlNifMutex *mu = xmalloc(sizeof *mu);
    pthread_mutex_init(&mu->m, NULL);
    mu->held = 0;
    snprintf(mu->name, sizeof mu->name, "%s", name ? name : "");
    pthread_mutex_lock(&G);
    mu->prev = NULL; mu->next = mutexes;
    if (mutexes) mutexes->prev = mu;
    mutexes = mu;
    n_mutexes++;
    pthread_mutex_unlock(&G);
    return mu;
}

void enif_mutex_destroy(ErlNifMutex *mu) {
    if (!mu) die("enif_mutex_destroy(NULL)");
    if (mu->held) die("enif_mutex_destroy of a held mutex");
    pthread_mutex_lock(&G);
    if (mu->prev) mu->prev->next = mu->next; else mutexes = mu->next;
    if (mu->next) mu->next->prev = mu->prev;
    n_mutexes--;
    pthread_mutex_unlock(&G);
    pthread_mutex_destroy(&mu->m);
    free(mu);
}

int enif_mutex_trylock(ErlNifMutex *mu) {
    if (!mu) die("enif_mutex_trylock(NULL)");
    pthread_mutex_lock(&G);
    int b = busy_next;
    busy_next = 0;
    pthread_mutex_unlock(&G);
    if (b) return EBUSY;
    if (pthread_mutex_trylock(&mu->m) != 0) return EBUSY;
    mu->owner = pthread_self();
    mu->held = 1;
    return 0;
}

void enif_mutex_lock(ErlNifMutex *mu) {
    if (!mu) die("enif_mutex_lock(NULL)");
    if (mu->held && pthread_equal(mu->owner, pthread_self())) die("enif_mutex_lock of a mutex the thread holds");
    pthread_mutex_lock(&mu->m);
    mu->owner = pthread_self();
    mu->held = 1;
}

void enif_mutex_unlock(ErlNifMutex *mu) {
    if (!mu) die("enif_mutex_unlock(NULL)");
    if (!mu->held || !pthread_equal(mu->owner, pthread_self()))
        die("enif_mutex_unlock of a mutex the calling thread does not hold");
    mu->held = 0;
    pthread_mutex_unlock(&mu->m);
}

/* ---------------------------------------------------------------- terms -- */
static char *atoms[4096];
static unsigned n_atoms;

ERL_NIF_TERM enif_make_atom(ErlNifEnv *env, const char *name) {
    if (!name) die("enif_make_atom(NULL)");
    if (strlen(name) > 255) die("enif_make_atom: a name of %zu bytes (at most 255)", strlen(name));
    pthread_mutex_lock(&G);
    unsigned k = 0;
    while (k < n_atoms && strcmp(atoms[k], name)) k++;
    if (k == n_atoms) {
        if (n_atoms == 4096) die("atom table full");
        atoms[n_atoms] = xmalloc(strlen(name) + 1);
        strcpy(atoms[n_atoms++], name);
    }
    pthread_mutex_unlock(&G);
    term v = {T_ATOM, 0, k, NULL, NULL};
    return new_term(v);
}

ERL_NIF_TERM enif_make_uint64(ErlNifEnv *env, ErlNifUInt64 i) {
    term v = {T_INT, 0, i, NULL, NULL};
    return new_term(v);
}
ERL_NIF_TERM enif_make_uint(ErlNifEnv *env, unsigned i) { return enif_make_uint64(env, i); }

int enif_get_uint64(ErlNifEnv *env, ERL_NIF_TERM t, ErlNifUInt64 *ip) {
    term *x = T(t);
    if (x->kind != T_INT) return 0;
    *ip = x->u;
    return 1;
}
int enif_get_uint(ErlNifEnv *env, ERL_NIF_TERM t, unsigned *ip) {
    term *x = T(t);
    if (x->kind != T_INT || x->u > 0xFFFFFFFFull) return 0;
    *ip = (unsigned)x->u;
    return 1;
}
int enif_get_int(ErlNifEnv *env, ERL_NIF_TERM t, int *ip) {
    term *x = T(t);
    if (x->kind != T_INT || x->u > 0x7FFFFFFFull) return 0;
    *ip = (int)x->u;
    return 1;
}

ERL_NIF_TERM enif_make_badarg(ErlNifEnv *env) {
    env->exception = 1;
    return enif_make_atom(env, "badarg");
}

ERL_NIF_TERM fe_make_tuple(const ERL_NIF_TERM *e, unsigned n) {
    ERL_NIF_TERM *c = xmalloc(n * sizeof *c);
    for (unsigned i = 0; i < n; i++) { T(e[i]); c[i] = e[i]; }
    term v = {T_TUPLE, n, 0, c, NULL};
    return new_term(v);
}
ERL_NIF_TERM enif_make_tuple2(ErlNifEnv *env, ERL_NIF_TERM a, ERL_NIF_TERM b) {
    ERL_NIF_TERM e[2] = {a, b};
    return fe_make_tuple(e, 2);
}
ERL_NIF_TERM enif_make_tuple3(ErlNifEnv *env, ERL_NIF_TERM a, ERL_NIF_TERM b, ERL_NIF_TERM c) {
    ERL_NIF_TERM e[3] = {a, b, c};
    return fe_make_tuple(e, 3);
}
ERL_NIF_TERM enif_make_tuple4(ErlNifEnv *env, ERL_NIF_TERM a, ERL_NIF_TERM b, ERL_NIF_TERM c, ERL_NIF_TERM d) {
    ERL_NIF_TERM e[4] = {a, b, c, d};
    return fe_make_tuple(e, 4);
}

static ERL_NIF_TERM nil(void) {
    term v = {T_NIL, 0, 0, NULL, NULL};
    return new_term(v);
}
ERL_NIF_TERM enif_make_list_cell(ErlNifEnv *env, ERL_NIF_TERM car, ERL_NIF_TERM cdr) {
    T(car);
    if (T(cdr)->kind != T_NIL && T(cdr)->kind != T_CONS) die("enif_make_list_cell: an improper list");
    ERL_NIF_TERM *c = xmalloc(2 * sizeof *c);
    c[0] = car; c[1] = cdr;
    term v = {T_CONS, 2, 0, c, NULL};
    return new_term(v);
}
ERL_NIF_TERM enif_make_list_from_array(ErlNifEnv *env, const ERL_NIF_TERM arr[], unsigned cnt) {
    ERL_NIF_TERM l = nil();
    for (unsigned i = cnt; i-- > 0;) l = enif_make_list_cell(env, arr[i], l);
    return l;
}
ERL_NIF_TERM enif_make_list(ErlNifEnv *env, unsigned cnt, ...) {
    ERL_NIF_TERM arr[64];
    if (cnt > 64) die("enif_make_list: more than 64 elements");
    va_list ap;
    va_start(ap, cnt);
    for (unsigned i = 0; i < cnt; i++) arr[i] = va_arg(ap, ERL_NIF_TERM);
    va_end(ap);
    return enif_make_list_from_array(env, arr, cnt);
}

static int same(ERL_NIF_TERM a, ERL_NIF_TERM b) {
    term *x = T(a), *y = T(b);
    if (x->kind != y->kind) return 0;
    if (x->kind == T_INT || x->kind == T_ATOM) return x->u == y->u;
    die("a map key that is neither an atom nor an integer");
    return 0;
}

ERL_NIF_TERM enif_make_new_map(ErlNifEnv *env) {
    term v = {T_MAP, 0, 0, NULL, NULL};
    return new_term(v);
}
int enif_is_map(ErlNifEnv *env, ERL_NIF_TERM t) { return T(t)->kind == T_MAP; }

int enif_get_map_value(ErlNifEnv *env, ERL_NIF_TERM map, ERL_NIF_TERM key, ERL_NIF_TERM *value) {
    term *m = T(map);
    if (m->kind != T_MAP) return 0;
    ERL_NIF_TERM *kv = m->p;
    for (uint32_t i = 0; i < m->n; i++)
        if (same(kv[2 * i], key)) { *value = kv[2 * i + 1]; return 1; }
    return 0;
}

/* replaces an existing key's value, as maps:put/3 */
int enif_make_map_put(ErlNifEnv *env, ERL_NIF_TERM map_in, ERL_NIF_TERM key, ERL_NIF_TERM value,
                      ERL_NIF_TERM *map_out) {
    term *m = T(map_in);
    if (m->kind != T_MAP) return 0;
    T(value);
    uint32_t n = m->n, at = n;
    ERL_NIF_TERM *old = m->p, *kv = xmalloc((size_t)(n + 1) * 2 * sizeof *kv);
    for (uint32_t i = 0; i < n; i++) {
        kv[2 * i] = old[2 * i]; kv[2 * i + 1] = old[2 * i + 1];
        if (same(old[2 * i], key)) at = i;
    }
    kv[2 * at] = key; kv[2 * at + 1] = value;
    term v = {T_MAP, at == n ? n + 1 : n, 0, kv, NULL};
    *map_out = new_term(v);
    return 1;
}

int fe_map_put(ERL_NIF_TERM map, ERL_NIF_TERM key, ERL_NIF_TERM value, ERL_NIF_TERM *out) {
    ERL_NIF_TERM v;
    if (enif_get_map_value(NULL, map, key, &v)) return 0;
    return enif_make_map_put(NULL, map, key, value, out);
}

int fe_ok_payload(ERL_NIF_TERM t, ERL_NIF_TERM *x) {
    term *v = T(t);
    if (v->kind != T_TUPLE || v->n != 2) return 0;
    ERL_NIF_TERM *e = v->p;
    if (T(e[0])->kind != T_ATOM || strcmp(atoms[T(e[0])->u], "ok")) return 0;
    *x = e[1];
    return 1;
}

/* -------------------------------------------------------------- printing -- */
static void print_atom(FILE *f, const char *s) {
    int plain = s[0] >= 'a' && s[0] <= 'z';
    for (const char *c = s; *c && plain; c++)
        plain = (*c >= 'a' && *c <= 'z') || (*c >= 'A' && *c <= 'Z') || (*c >= '0' && *c <= '9') || *c == '_' || *c == '@';
    if (plain) { fputs(s, f); return; }
    fputc('\'', f);
    for (const char *c = s; *c; c++) {
        if (*c == '\'' || *c == '\\') fputc('\\', f);
        fputc(*c, f);
    }
    fputc('\'', f);
}

void fe_print(FILE *f, ERL_NIF_TERM t) {
    term *x = T(t);
    ERL_NIF_TERM *e = x->p;
    switch (x->kind) {
    case T_INT: fprintf(f, "%llu", (unsigned long long)x->u); break;
    case T_ATOM: print_atom(f, atoms[x->u]); break;
    case T_TUPLE:
        fputc('{', f);
        for (uint32_t i = 0; i < x->n; i++) { if (i) fputc(',', f); fe_print(f, e[i]); }
        fputc('}', f);
        break;
    case T_NIL: fputs("[]", f); break;
    case T_CONS:
        fputc('[', f);
        for (int first = 1; x->kind == T_CONS; x = T(((ERL_NIF_TERM *)x->p)[1]), first = 0) {
            if (!first) fputc(',', f);
            fe_print(f, ((ERL_NIF_TERM *)x->p)[0]);
        }
        fputc(']', f);
        break;
    case T_MAP:
        fputs("#{", f);
        for (uint32_t i = 0; i < x->n; i++) {
            if (i) fputc(',', f);
            fe_print(f, e[2 * i]); fputs("=>", f); fe_print(f, e[2 * i + 1]);
        }
        fputc('}', f);
        break;
    case T_BIN: {
        static const char hex[] = "0123456789abcdef";
        const unsigned char *d = x->p;
        fputs("<<", f);
        for (uint64_t i = 0; i < x->u; i++) { fputc(hex[d[i] >> 4], f); fputc(hex[d[i] & 15], f); }
        fputs(">>", f);
        break;
    }
    default: fprintf(f, "'#Ref<%ld>'", ((rhdr *)x->p - 1)->serial); break;
    }
}

/* ------------------------------------------------------------- the arena -- */
size_t fe_mark(void) {
    pthread_mutex_lock(&G);
    size_t m = top;
    pthread_mutex_unlock(&G);
    return m;
}

void fe_release(size_t mark) {
    for (;;) {
        pthread_mutex_lock(&G);
        if (top <= mark) { pthread_mutex_unlock(&G); return; }
        size_t i = --top;
        term v = chunks[i / CHUNK][i % CHUNK];
        pthread_mutex_unlock(&G);
        if (v.kind == T_RES) enif_release_resource(v.p);       /* (may run the destructor) */
        else if (v.kind == T_BIN) free(v.base);
        else free(v.p);
    }
}

/* ----------------------------------------------------------- accounting -- */
fe_live_t fe_live(void) {
    fe_live_t l;
    pthread_mutex_lock(&G);
    l.allocs = n_allocs; l.binaries = n_owned; l.resources = n_resources; l.mutexes = n_mutexes;
    l.held_by_me = 0;
    for (ErlNifMutex *m = mutexes; m; m = m->next)
        if (m->held && pthread_equal(m->owner, pthread_self())) l.held_by_me++;
    pthread_mutex_unlock(&G);
    return l;
}

long fe_report_leaks(FILE *f) {
    long n = 0;
    pthread_mutex_lock(&G);
    for (ahdr *a = allocs; a; a = a->next, n++) fprintf(f, "leak: enif_alloc #%ld of %zu bytes\n", a->serial, a->size);
    for (brec *b = brecs; b; b = b->next)
        if (b->state == B_OWNED) { fprintf(f, "leak: binary #%ld of %zu bytes neither made nor released\n", b->serial, b->size); n++; }
    for (rhdr *r = resources; r; r = r->next, n++)
        fprintf(f, "leak: resource #%ld (%s) with %ld references\n", r->serial, r->type->name, r->refc);
    for (ErlNifMutex *m = mutexes; m; m = m->next, n++) fprintf(f, "leak: mutex %s%s\n", m->name, m->held ? " (held)" : "");
    pthread_mutex_unlock(&G);
    return n;
}
