/* tests/stubs/mex_runtime.c -- a small working implementation of the part of MATLAB's mex API that
 * em_model_manned_bayes_amd/matlab/emgpu_mex.c uses (every function tests/stubs/mex.h declares), so that the tests can RUN the
 * gateway without MATLAB: tests/mexrt.py compiles this file together with emgpu_mex.c into one shared object and drives
 * mexFunction through rt_call().  Test infrastructure only; it keeps to MATLAB's documented behaviour where the gateway can
 * depend on it, and it is stricter than MATLAB where a mistake would otherwise go unseen:
 *   - mxCreate* and mxCalloc zero-fill; mxMalloc fills with 0xA5 (MATLAB leaves it uninitialised)
 *   - every data block has guard words on both sides, checked on mxFree, on destruction and by rt_check_guards()
 *   - an index or a field name outside an array, mxGetPr on a non-double array, mxFree of a foreign pointer and a plhs slot written
 *     beyond max(nlhs, 1) are recorded as violations (rt_violations())
 *   - mexErrMsgIdAndTxt stores identifier and text, frees what the call allocated (as MATLAB does) and longjmps to rt_call
 */
#include <setjmp.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mex.h"

#define RT_GUARD_WORDS 4096 /* 32 KiB on each side: an overrun by a whole row of a batch still lands in the guard, not in the heap */
#define RT_GUARD 0xC0FFEE5AFEC0DE11ull
#define RT_MAGIC 0x6D786172u /* 'mxar' */
#define RT_MAX_DIMS 8
#define RT_SENTINELS 8

enum { RT_LOGICAL_CLASS = 3, RT_CHAR_CLASS = 4, RT_CELL_CLASS = 1, RT_STRUCT_CLASS = 2 }; /* MATLAB's own mxClassID values */

/* a guarded block: [header][guard words][payload][guard words] */
typedef struct rt_block {
    uint32_t magic;
    int is_malloc;          /* a mxMalloc / mxCalloc block (freed when the call errors) or an array payload */
    uint64_t epoch;         /* the rt_call during which it was made */
    size_t size;
    struct rt_block *prev, *next;
} rt_block;

struct mxArray_tag {
    int classid;
    size_t ndim;
    size_t dims[RT_MAX_DIMS];
    void *data;             /* guarded payload: elements, or mxArray* per cell / per (element, field) */
    int nfields;
    char **fieldnames;
    uint64_t epoch;
    int mark;
    struct mxArray_tag *prev, *next;
};

static rt_block *g_blocks = NULL;
static mxArray *g_arrays = NULL;
static uint64_t g_epoch = 0;
static int g_in_call = 0;
static jmp_buf g_jmp;
static char g_err_id[256], g_err_msg[4096];
static char g_viol[8192];
static int g_nviol = 0;
static void (*g_at_exit)(void) = NULL;
static int g_at_exit_registrations = 0;

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]);

static void violation(const char *fmt, ...) {
    char line[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    g_nviol++;
    const size_t used = strlen(g_viol);
    if (used + strlen(line) + 2 < sizeof g_viol) { strcat(g_viol, line); strcat(g_viol, "\n"); }
}

/* ---- guarded blocks */
static uint64_t *guard_before(rt_block *b) { return (uint64_t *)(b + 1); }
static unsigned char *payload(rt_block *b) { return (unsigned char *)(guard_before(b) + RT_GUARD_WORDS); }
static rt_block *block_of(void *p) { return (rt_block *)((uint64_t *)p - RT_GUARD_WORDS) - 1; }

static void *block_new(size_t size, int is_malloc, int fill) {
    rt_block *b = (rt_block *)malloc(sizeof(rt_block) + 2 * RT_GUARD_WORDS * sizeof(uint64_t) + size);
    if (!b) abort();
    b->magic = RT_MAGIC; b->is_malloc = is_malloc; b->epoch = g_epoch; b->size = size;
    b->prev = NULL; b->next = g_blocks;
    if (g_blocks) g_blocks->prev = b;
    g_blocks = b;
    const uint64_t g = RT_GUARD;
    for (int i = 0; i < RT_GUARD_WORDS; i++) guard_before(b)[i] = g;
    memset(payload(b), fill, size);
    for (int i = 0; i < RT_GUARD_WORDS; i++) memcpy(payload(b) + size + i * sizeof g, &g, sizeof g);   /* may be unaligned */
    return payload(b);
}

static int block_check(rt_block *b, const char *when) {
    int bad = 0;
    const uint64_t g = RT_GUARD;
    for (int i = 0; i < RT_GUARD_WORDS; i++) {
        if (guard_before(b)[i] != g) bad |= 1;
        if (memcmp(payload(b) + b->size + i * sizeof g, &g, sizeof g)) bad |= 2;
    }
    if (bad) violation("%s: %s block of %zu bytes overwritten %s%s", when, b->is_malloc ? "mxMalloc" : "array", b->size,
                       bad & 1 ? "before its start " : "", bad & 2 ? "past its end" : "");
    return bad != 0;
}

static void block_free(void *p, const char *when) {
    rt_block *b = block_of(p);
    block_check(b, when);
    if (b->prev) b->prev->next = b->next; else g_blocks = b->next;
    if (b->next) b->next->prev = b->prev;
    b->magic = 0;
    free(b);
}

void *mxMalloc(size_t n) { return block_new(n, 1, 0xA5); }
void *mxCalloc(size_t n, size_t size) { return block_new(n * size, 1, 0); }
void mxFree(void *p) {
    if (!p) return;
    rt_block *b = block_of(p);
    if (b->magic != RT_MAGIC || !b->is_malloc) { violation("mxFree of a pointer that mxMalloc / mxCalloc did not return"); return; }
    block_free(p, "mxFree");
}

/* ---- arrays */
static size_t elsize(int c) {
    switch (c) {
    case mxDOUBLE_CLASS: case mxUINT64_CLASS: return 8;
    case mxUINT8_CLASS: case RT_LOGICAL_CLASS: return 1;
    case RT_CHAR_CLASS: return 2;
    default: return sizeof(mxArray *);
    }
}

static size_t numel(const mxArray *a) {
    size_t n = 1;
    for (size_t i = 0; i < a->ndim; i++) n *= a->dims[i];
    return n;
}

static mxArray *array_new(int classid, size_t ndim, const size_t *dims, int nfields) {
    mxArray *a = (mxArray *)calloc(1, sizeof *a);
    if (!a) abort();
    a->classid = classid;
    a->ndim = ndim < 2 ? 2 : ndim;
    if (a->ndim > RT_MAX_DIMS) { violation("array with %zu dimensions", ndim); a->ndim = RT_MAX_DIMS; }
    a->dims[0] = a->dims[1] = 1;
    for (size_t i = 0; i < ndim && i < RT_MAX_DIMS; i++) a->dims[i] = dims[i];
    while (a->ndim > 2 && a->dims[a->ndim - 1] == 1) a->ndim--;       /* MATLAB drops trailing singleton dimensions */
    a->nfields = nfields;
    a->data = block_new(numel(a) * elsize(classid) * (classid == RT_STRUCT_CLASS ? (size_t)nfields : 1), 0, 0);
    a->epoch = g_epoch;
    a->next = g_arrays;
    if (g_arrays) g_arrays->prev = a;
    g_arrays = a;
    return a;
}

static void array_free_one(mxArray *a) {
    block_free(a->data, "array destruction");
    for (int i = 0; i < a->nfields; i++) free(a->fieldnames[i]);
    free(a->fieldnames);
    if (a->prev) a->prev->next = a->next; else g_arrays = a->next;
    if (a->next) a->next->prev = a->prev;
    free(a);
}

static size_t n_children(const mxArray *a) {
    if (a->classid == RT_CELL_CLASS) return numel(a);
    if (a->classid == RT_STRUCT_CLASS) return numel(a) * (size_t)a->nfields;
    return 0;
}

void rt_destroy(mxArray *a) {          /* mxDestroyArray: the array and everything it holds */
    if (!a) return;
    const size_t n = n_children(a);
    for (size_t i = 0; i < n; i++) rt_destroy(((mxArray **)a->data)[i]);
    array_free_one(a);
}

mxArray *mxCreateNumericArray(mwSize nd, const mwSize *dims, mxClassID c, mxComplexity f) { (void)f; return array_new((int)c, nd, dims, 0); }
mxArray *mxCreateNumericMatrix(mwSize m, mwSize n, mxClassID c, mxComplexity f) { const size_t d[2] = {m, n}; (void)f; return array_new((int)c, 2, d, 0); }
mxArray *mxCreateDoubleMatrix(mwSize m, mwSize n, mxComplexity f) { return mxCreateNumericMatrix(m, n, mxDOUBLE_CLASS, f); }
mxArray *mxCreateDoubleScalar(double v) { mxArray *a = mxCreateDoubleMatrix(1, 1, mxREAL); *(double *)a->data = v; return a; }
mxArray *mxCreateLogicalMatrix(mwSize m, mwSize n) { const size_t d[2] = {m, n}; return array_new(RT_LOGICAL_CLASS, 2, d, 0); }
mxArray *mxCreateCellMatrix(mwSize m, mwSize n) { const size_t d[2] = {m, n}; return array_new(RT_CELL_CLASS, 2, d, 0); }
mxArray *mxCreateStructMatrix(mwSize m, mwSize n, int nfields, const char **fieldnames) {
    const size_t d[2] = {m, n};
    mxArray *a = array_new(RT_STRUCT_CLASS, 2, d, nfields);
    a->fieldnames = (char **)calloc((size_t)(nfields > 0 ? nfields : 1), sizeof(char *));
    for (int i = 0; i < nfields; i++) {
        a->fieldnames[i] = (char *)malloc(strlen(fieldnames[i]) + 1);
        strcpy(a->fieldnames[i], fieldnames[i]);
    }
    return a;
}
mxArray *mxCreateString(const char *s) {
    const size_t len = strlen(s);
    const size_t d[2] = {len ? 1 : 0, len};                  /* '' is 0 x 0 */
    mxArray *a = array_new(RT_CHAR_CLASS, 2, d, 0);
    for (size_t i = 0; i < len; i++) ((uint16_t *)a->data)[i] = (unsigned char)s[i];
    return a;
}

size_t mxGetNumberOfElements(const mxArray *a) { return numel(a); }
size_t mxGetM(const mxArray *a) { return a->dims[0]; }
size_t mxGetN(const mxArray *a) { size_t n = 1; for (size_t i = 1; i < a->ndim; i++) n *= a->dims[i]; return n; }
int mxIsEmpty(const mxArray *a) { return numel(a) == 0; }
int mxIsChar(const mxArray *a) { return a->classid == RT_CHAR_CLASS; }
int mxIsLogical(const mxArray *a) { return a->classid == RT_LOGICAL_CLASS; }
int mxIsDouble(const mxArray *a) { return a->classid == mxDOUBLE_CLASS; }
int mxIsCell(const mxArray *a) { return a->classid == RT_CELL_CLASS; }
int mxIsStruct(const mxArray *a) { return a->classid == RT_STRUCT_CLASS; }
void *mxGetData(const mxArray *a) { return a->data; }
double *mxGetPr(const mxArray *a) {
    if (a->classid != mxDOUBLE_CLASS) violation("mxGetPr of an array of class %d", a->classid);
    return (double *)a->data;
}
unsigned char *mxGetLogicals(const mxArray *a) {
    if (a->classid != RT_LOGICAL_CLASS) { violation("mxGetLogicals of an array of class %d", a->classid); return NULL; }
    return (unsigned char *)a->data;
}
int mxIsLogicalScalarTrue(const mxArray *a) { return a->classid == RT_LOGICAL_CLASS && numel(a) == 1 && *(unsigned char *)a->data != 0; }
double mxGetScalar(const mxArray *a) {
    if (numel(a) == 0 || n_children(a)) { violation("mxGetScalar of an empty, cell or struct array"); return 0.0; }
    switch (a->classid) {
    case mxDOUBLE_CLASS: return *(double *)a->data;
    case mxUINT64_CLASS: return (double)*(uint64_t *)a->data;
    case RT_CHAR_CLASS: return (double)*(uint16_t *)a->data;
    default: return (double)*(unsigned char *)a->data;
    }
}
int mxGetString(const mxArray *a, char *buf, mwSize n) {
    if (a->classid != RT_CHAR_CLASS || n == 0) return 1;
    const size_t len = numel(a), k = len < n - 1 ? len : n - 1;
    for (size_t i = 0; i < k; i++) buf[i] = (char)((uint16_t *)a->data)[i];
    buf[k] = 0;
    return len > n - 1;
}

mxArray *mxGetCell(const mxArray *a, mwSize i) {
    if (a->classid != RT_CELL_CLASS || i >= numel(a)) { violation("mxGetCell index %zu outside a cell array of %zu", (size_t)i, numel(a)); return NULL; }
    return ((mxArray **)a->data)[i];
}
void mxSetCell(mxArray *a, mwSize i, mxArray *v) {
    if (a->classid != RT_CELL_CLASS || i >= numel(a)) { violation("mxSetCell index %zu outside a cell array of %zu", (size_t)i, numel(a)); return; }
    ((mxArray **)a->data)[i] = v;
}
static int field_number(const mxArray *a, const char *name) {
    for (int f = 0; f < a->nfields; f++) if (!strcmp(a->fieldnames[f], name)) return f;
    return -1;
}
mxArray *mxGetField(const mxArray *a, mwSize i, const char *name) {   /* an absent field is NULL, as documented */
    if (a->classid != RT_STRUCT_CLASS || i >= numel(a)) { violation("mxGetField index %zu outside a struct array", (size_t)i); return NULL; }
    const int f = field_number(a, name);
    return f < 0 ? NULL : ((mxArray **)a->data)[i * (size_t)a->nfields + (size_t)f];
}
void mxSetField(mxArray *a, mwSize i, const char *name, mxArray *v) {
    const int f = a->classid == RT_STRUCT_CLASS ? field_number(a, name) : -1;
    if (f < 0 || i >= numel(a)) { violation("mxSetField of '%s', element %zu: no such field or element", name, (size_t)i); return; }
    ((mxArray **)a->data)[i * (size_t)a->nfields + (size_t)f] = v;
}

int mexAtExit(void (*fn)(void)) { g_at_exit = fn; g_at_exit_registrations++; return 0; }

/* everything the running call allocated goes, as in MATLAB, when it ends with an error */
static void release_call(int arrays_too) {
    for (rt_block *b = g_blocks, *nx; b; b = nx) {
        nx = b->next;
        if (b->is_malloc && b->epoch == g_epoch) block_free(payload(b), "release at the end of a call");
    }
    if (!arrays_too) return;
    for (mxArray *a = g_arrays, *nx; a; a = nx) {
        nx = a->next;
        if (a->epoch == g_epoch) array_free_one(a);
    }
}

void mexErrMsgIdAndTxt(const char *id, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err_msg, sizeof g_err_msg, fmt, ap);
    va_end(ap);
    snprintf(g_err_id, sizeof g_err_id, "%s", id);
    if (!g_in_call) { fprintf(stderr, "mexErrMsgIdAndTxt outside rt_call: %s: %s\n", g_err_id, g_err_msg); abort(); }
    release_call(1);
    longjmp(g_jmp, 1);
}

/* ---- what tests/mexrt.py calls */
static void mark(mxArray *a) {
    if (!a || a->mark) return;
    a->mark = 1;
    const size_t n = n_children(a);
    for (size_t i = 0; i < n; i++) mark(((mxArray **)a->data)[i]);
}

static mxArray g_sentinel;

/* 0: returned, 1: mexErrMsgIdAndTxt (rt_error_id / rt_error_msg).  plhs: room for max(nlhs, 1) results. */
int rt_call(int nlhs, mxArray **plhs, int nrhs, const mxArray **prhs) {
    const int real = nlhs > 1 ? nlhs : 1;
    mxArray **slots = (mxArray **)calloc((size_t)(real + RT_SENTINELS), sizeof *slots);
    for (int i = 0; i < RT_SENTINELS; i++) slots[real + i] = &g_sentinel;
    g_epoch++;
    g_err_id[0] = g_err_msg[0] = 0;
    g_in_call = 1;
    int rc = 0;
    if (setjmp(g_jmp) == 0) mexFunction(nlhs, slots, nrhs, prhs); else rc = 1;
    g_in_call = 0;
    for (int i = 0; i < RT_SENTINELS; i++)
        if (slots[real + i] != &g_sentinel) violation("plhs[%d] written with nlhs = %d", real + i, nlhs);
    for (int i = 0; i < real; i++) plhs[i] = rc ? NULL : slots[i];
    if (!rc) {
        /* MATLAB destroys the arrays a call created and did not return, and frees the mxMalloc blocks it left */
        int left = 0;
        for (rt_block *b = g_blocks; b; b = b->next) left += b->is_malloc && b->epoch == g_epoch;
        if (left) violation("%d mxMalloc block(s) not freed when the call returned", left);
        release_call(0);
        for (int i = 0; i < real; i++) mark(slots[i]);
        for (mxArray *a = g_arrays, *nx; a; a = nx) {
            nx = a->next;
            if (a->epoch == g_epoch && !a->mark) array_free_one(a);
        }
        for (mxArray *a = g_arrays; a; a = a->next) a->mark = 0;
    }
    free(slots);
    return rc;
}

const char *rt_error_id(void) { return g_err_id; }
const char *rt_error_msg(void) { return g_err_msg; }

int rt_check_guards(void) {          /* every live block; returns how many were overwritten */
    int bad = 0;
    for (rt_block *b = g_blocks; b; b = b->next) bad += block_check(b, "rt_check_guards");
    return bad;
}

int rt_violation_count(void) { return g_nviol; }
const char *rt_violations(void) { return g_viol; }
void rt_clear_violations(void) { g_nviol = 0; g_viol[0] = 0; }

int rt_live_arrays(void) { int n = 0; for (mxArray *a = g_arrays; a; a = a->next) n++; return n; }
int rt_live_blocks(void) { int n = 0; for (rt_block *b = g_blocks; b; b = b->next) n++; return n; }

int rt_at_exit_registrations(void) { return g_at_exit_registrations; }
int rt_run_at_exit(void) {          /* what MATLAB does when the mex file is cleared; 1 if a function was registered */
    void (*fn)(void) = g_at_exit;
    g_at_exit = NULL;
    if (fn) fn();
    return fn != NULL;
}

/* inspection and construction for the numpy conversion */
int rt_class(const mxArray *a) { return a->classid; }
int rt_ndim(const mxArray *a) { return (int)a->ndim; }
size_t rt_dim(const mxArray *a, int i) { return a->dims[i]; }
int rt_nfields(const mxArray *a) { return a->nfields; }
const char *rt_fieldname(const mxArray *a, int f) { return a->fieldnames[f]; }
mxArray *rt_new(int classid, int ndim, const size_t *dims) { return array_new(classid, (size_t)ndim, dims, 0); }
