/*
 * tests/nif_run/beam_main.c -- TEST INFRASTRUCTURE ONLY: a stand-alone driver
 * of erlang/c_src/partisan_gpu_sim_nif.c over the stand-in runtime
 * (fake_erts.c).  The shim is compiled into this program; nif_init() is an
 * ordinary function under tests/nif_lint/erl_nif.h's ERL_NIF_INIT.
 *
 * The program checks the function table, runs `load`, then reads a script
 * from stdin, one command a line, and answers every line with exactly one
 * line on stdout (flushed), so a parent may drive it interactively:
 *
 *   [name =] nif arg ...      call the NIF of that name and arity; prints the
 *                             result as Erlang term text (binaries as hex), or
 *                             `badarg` when the call raised, whatever it
 *                             returned.  With `name =`, $name is X of an
 *                             {ok, X} result, else the whole result.
 *   spawn name nif arg ...    the same call on a second thread; prints `spawned`
 *   await name                joins it; prints (and binds) its result
 *   !table                    [{Name, Arity, Flags}] of the function table
 *   !fail alloc|alloc_binary|alloc_resource|mutex_create K
 *                             the K-th such call from now fails
 *   !busy                     the next enif_mutex_trylock answers busy
 *   !align 0|1                binaries of later lines sit at an odd address (0,
 *                             the default) or an aligned one
 *   !other name               $name: a resource of another type
 *   !live                     what is alive: allocs, owned binaries, resources, mutexes
 *
 * Terms: integers, atoms (plain or 'quoted'), <<hex>>, {..}, [..],
 * #{k => v, ..}, $name.  After every call no mutex may be held by the calling
 * thread.  At the end of the script every term is dropped and everything must
 * be gone; otherwise the list goes to stderr and the exit status is 4.
 */
#include "fake_erts.h"

#include <ctype.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

ErlNifEntry *nif_init(void);

static ErlNifEntry *entry;
static int aligned;
static ErlNifEnv main_env;

typedef struct { char name[64]; ERL_NIF_TERM t; } var;
static var vars[256];
static int n_vars;

static void fatal(int code, const char *fmt, const char *a, const char *b) {
    fflush(stdout);
    fprintf(stderr, "beam_main: ");
    fprintf(stderr, fmt, a, b);
    fputc('\n', stderr);
    fflush(NULL);
    exit(code);
}

static void bind(const char *name, ERL_NIF_TERM t) {
    ERL_NIF_TERM x;
    if (fe_ok_payload(t, &x)) t = x;
    for (int i = 0; i < n_vars; i++)
        if (!strcmp(vars[i].name, name)) { vars[i].t = t; return; }
    if (n_vars == 256) fatal(2, "too many variables%s%s", "", "");
    snprintf(vars[n_vars].name, sizeof vars[n_vars].name, "%s", name);
    vars[n_vars++].t = t;
}

/* ---------------------------------------------------------------- parser -- */
static const char *P, *LINE;

static void ws(void) { while (*P == ' ' || *P == '\t') P++; }
static void bad(const char *what) { fatal(2, "script: %s at: %s", what, P); }

static int ident(char *out, size_t cap) {
    size_t n = 0;
    if (!(isalpha((unsigned char)*P) || *P == '_')) return 0;
    while (isalnum((unsigned char)*P) || *P == '_' || *P == '@') {
        if (n + 1 < cap) out[n++] = *P;
        P++;
    }
    out[n] = 0;
    return 1;
}

static ERL_NIF_TERM parse_term(void);

static unsigned parse_seq(char close, ERL_NIF_TERM *out, unsigned cap) {
    unsigned n = 0;
    ws();
    if (*P == close) { P++; return 0; }
    for (;;) {
        if (n == cap) bad("too many elements");
        out[n++] = parse_term();
        ws();
        if (*P == ',') { P++; continue; }
        if (*P == close) { P++; return n; }
        bad("expected , or a closing bracket");
    }
}

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

static ERL_NIF_TERM parse_term(void) {
    char name[300];
    ws();
    if (isdigit((unsigned char)*P)) {
        char *end;
        unsigned long long v = strtoull(P, &end, 10);
        P = end;
        return enif_make_uint64(&main_env, v);
    }
    if (*P == '$') {
        P++;
        if (!ident(name, sizeof name)) bad("a variable name");
        for (int i = 0; i < n_vars; i++)
            if (!strcmp(vars[i].name, name)) return vars[i].t;
        bad("an unbound variable");
    }
    if (*P == '\'') {
        size_t n = 0;
        for (P++; *P && *P != '\''; P++) {
            if (*P == '\\' && P[1]) P++;
            if (n + 1 < sizeof name) name[n++] = *P;
        }
        if (*P != '\'') bad("an unterminated atom");
        P++;
        name[n] = 0;
        return enif_make_atom(&main_env, name);
    }
    if (P[0] == '<' && P[1] == '<') {
        P += 2;
        const char *s = P;
        while (hexval(*P) >= 0) P++;
        size_t n = (size_t)(P - s);
        if (n % 2 || P[0] != '>' || P[1] != '>') bad("a binary is <<hex digits>>");
        unsigned char *b = malloc(n / 2 + 1);
        for (size_t i = 0; i < n / 2; i++) b[i] = (unsigned char)(hexval(s[2 * i]) << 4 | hexval(s[2 * i + 1]));
        P += 2;
        ERL_NIF_TERM t = fe_make_script_binary(b, n / 2, aligned);
        free(b);
        return t;
    }
    if (*P == '{') {
        ERL_NIF_TERM e[64];
        P++;
        unsigned n = parse_seq('}', e, 64);
        return fe_make_tuple(e, n);
    }
    if (*P == '[') {
        static ERL_NIF_TERM e[65536];
        P++;
        unsigned n = parse_seq(']', e, 65536);
        return enif_make_list_from_array(&main_env, e, n);
    }
    if (P[0] == '#' && P[1] == '{') {
        ERL_NIF_TERM m = enif_make_new_map(&main_env);
        P += 2;
        ws();
        if (*P == '}') { P++; return m; }
        for (;;) {
            ERL_NIF_TERM k = parse_term();
            ws();
            if (P[0] != '=' || P[1] != '>') bad("expected =>");
            P += 2;
            ERL_NIF_TERM v = parse_term();
            if (!fe_map_put(m, k, v, &m)) bad("a key twice in a map");
            ws();
            if (*P == ',') { P++; continue; }
            if (*P == '}') { P++; return m; }
            bad("expected , or }");
        }
    }
    if (ident(name, sizeof name)) return enif_make_atom(&main_env, name);
    bad("a term");
    return 0;
}

/* ----------------------------------------------------------------- calls -- */
typedef struct {
    ErlNifFunc *f;
    int argc;
    ERL_NIF_TERM argv[16];
    ErlNifEnv env;
    ERL_NIF_TERM result;
    long held;
} call;

static void run(call *c) {
    c->env.exception = 0;
    c->result = c->f->fptr(&c->env, c->argc, c->argv);
    c->held = fe_live().held_by_me;
}

static void *run_thread(void *p) { run((call *)p); return NULL; }

static void parse_call(call *c) {
    char nif[64];
    ws();
    if (!ident(nif, sizeof nif)) bad("a NIF name");
    c->argc = 0;
    for (ws(); *P; ws()) {
        if (c->argc == 16) bad("too many arguments");
        c->argv[c->argc++] = parse_term();
    }
    c->f = NULL;
    for (int i = 0; i < entry->num_of_funcs; i++)
        if (!strcmp(entry->funcs[i].name, nif) && (int)entry->funcs[i].arity == c->argc) c->f = &entry->funcs[i];
}

static void answer(call *c, const char *nif_line) {
    if (c->held) fatal(3, "a mutex is still held after: %s%s", nif_line, "");
    if (c->env.exception) fputs("badarg", stdout);
    else fe_print(stdout, c->result);
    fputc('\n', stdout);
}

static struct { int live; char name[64]; pthread_t th; call c; char line[256]; } bg;

static void directive(void) {
    char w[64], what[64];
    P++;
    if (!ident(w, sizeof w)) bad("a directive");
    ws();
    if (!strcmp(w, "table")) {
        fputc('[', stdout);
        for (int i = 0; i < entry->num_of_funcs; i++)
            printf("%s{%s,%u,%u}", i ? "," : "", entry->funcs[i].name, entry->funcs[i].arity, entry->funcs[i].flags);
        puts("]");
        return;
    }
    if (!strcmp(w, "fail")) {
        static const char *names[FE_NFAIL] = {"alloc", "alloc_binary", "alloc_resource", "mutex_create"};
        if (!ident(what, sizeof what)) bad("what fails");
        int k = -1;
        for (int i = 0; i < FE_NFAIL; i++)
            if (!strcmp(what, names[i])) k = i;
        if (k < 0) bad("an unknown failure point");
        fe_fail(k, (unsigned)strtoul(P, NULL, 10));
    } else if (!strcmp(w, "busy")) {
        fe_busy_next_trylock();
    } else if (!strcmp(w, "align")) {
        aligned = atoi(P) != 0;
    } else if (!strcmp(w, "other")) {
        static ErlNifResourceType *other;
        if (!ident(what, sizeof what)) bad("a variable name");
        if (!other) other = enif_open_resource_type(&main_env, NULL, "other", NULL, ERL_NIF_RT_CREATE, NULL);
        void *obj = enif_alloc_resource(other, 8);
        bind(what, enif_make_resource(&main_env, obj));
        enif_release_resource(obj);
    } else if (!strcmp(w, "live")) {
        fe_live_t l = fe_live();
        printf("{live,%ld,%ld,%ld,%ld}\n", l.allocs, l.binaries, l.resources, l.mutexes);
        return;
    } else {
        bad("an unknown directive");
    }
    puts("ok");
}

int main(void) {
    entry = nif_init();
    if (!entry || strcmp(entry->name, "partisan_gpu_sim") || entry->num_of_funcs <= 0 || !entry->funcs || !entry->load)
        fatal(2, "nif_init: a malformed entry%s%s", "", "");
    for (int i = 0; i < entry->num_of_funcs; i++) {
        ErlNifFunc *f = &entry->funcs[i];
        if (!f->name || !f->name[0] || !f->fptr || f->arity > 16 || f->flags > ERL_NIF_DIRTY_JOB_IO_BOUND)
            fatal(2, "function table: a malformed entry %s%s", f->name ? f->name : "?", "");
        for (int j = 0; j < i; j++)
            if (!strcmp(entry->funcs[j].name, f->name) && entry->funcs[j].arity == f->arity)
                fatal(2, "function table: %s twice%s", f->name, "");
    }
    void *priv = NULL;
    if (entry->load(&main_env, &priv, enif_make_atom(&main_env, "undefined")) != 0) fatal(2, "load failed%s%s", "", "");

    char *line = NULL;
    size_t cap = 0;
    ssize_t len;
    size_t keep = fe_mark();
    while ((len = getline(&line, &cap, stdin)) > 0) {
        while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r' || line[len - 1] == ' ')) line[--len] = 0;
        P = LINE = line;
        ws();
        if (!*P || *P == '%') { puts("ok"); fflush(stdout); continue; }
        size_t mark = fe_mark();
        int bound = 0;
        if (*P == '!') {
            directive();
            bound = 1;              /* (!other binds) */
        } else {
            char first[64], name[64] = "";
            const char *start = P;
            if (!ident(first, sizeof first)) bad("a command");
            ws();
            if (!strcmp(first, "await")) {
                if (!ident(name, sizeof name) || !bg.live || strcmp(name, bg.name)) bad("nothing spawned under that name");
                pthread_join(bg.th, NULL);
                bg.live = 0;
                answer(&bg.c, bg.line);
                bind(name, bg.c.result);
                bound = 1;
            } else if (!strcmp(first, "spawn")) {
                if (bg.live) bad("a call is already spawned");
                if (!ident(bg.name, sizeof bg.name)) bad("a name");
                snprintf(bg.line, sizeof bg.line, "%s", P);
                parse_call(&bg.c);
                if (!bg.c.f) bad("no such NIF at that arity");
                bg.live = 1;
                if (pthread_create(&bg.th, NULL, run_thread, &bg.c)) fatal(2, "pthread_create failed%s%s", "", "");
                puts("spawned");
                bound = 1;
            } else {
                if (*P == '=' && P[1] != '>') {
                    snprintf(name, sizeof name, "%s", first);
                    P++;
                } else {
                    P = start;
                }
                call c;
                const char *what = P;
                parse_call(&c);
                if (!c.f) {
                    printf("{undef,%d}\n", c.argc);
                } else {
                    run(&c);
                    answer(&c, what);
                    if (name[0]) { bind(name, c.result); bound = 1; }
                }
            }
        }
        fflush(stdout);
        if (bound) keep = fe_mark();
        else if (!bg.live) fe_release(mark > keep ? mark : keep);
    }
    free(line);
    if (bg.live) { pthread_join(bg.th, NULL); if (bg.c.held) fatal(3, "a mutex is still held after: %s%s", bg.line, ""); }
    n_vars = 0;
    fe_release(0);
    if (fe_report_leaks(stderr)) { fflush(NULL); return 4; }
    puts("{exit,clean}");
    return 0;
}
