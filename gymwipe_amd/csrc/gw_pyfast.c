/* gw_pyfast.c -- the per-step call from Python without ctypes.
 *
 * env.step() is enqueued about 200 000 times a second; through ctypes each call converts seven Python ints into C arguments
 * by way of generic descriptors (~1 us).  This CPython extension does the same call through METH_FASTCALL (~0.1 us).  It holds
 * no logic: it calls the C-ABI entry points whose addresses the Python side hands it (taken from the loaded
 * libgymwipe_amd.so with ctypes), so it links against nothing but libpython's ABI and cannot drift from the library.
 * Built in-tree by the Makefile next to the library; gymwipe_amd/_native.py falls back to ctypes when it is absent.
 *
 * Stepper (below) is VecCounterTrafficEnv.step's common case as ONE native call: the flat Python body around the launch
 * (two dict probes, the device test, the stream getter, the result tuple) cost 0.6-0.7 us of a 4 us enqueue. */
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <stddef.h>
#include <stdint.h>
#include <structmember.h>

typedef int (*gw_step_fn)(void*, const int32_t*, const int32_t*, int32_t*, float*, uint8_t*, void*);
typedef int (*gw_pend_fn)(void*, void*, const int32_t*, const int32_t*, int32_t*, float*, double*, void*);
typedef int (*gw_step_fb_fn)(void*, const int32_t*, const int32_t*, int32_t*, float*, uint8_t*, uint8_t*, void*);
static gw_step_fn g_step = NULL;
static gw_pend_fn g_pend = NULL;
typedef int (*gw_reset_fn)(void*, const uint8_t*, int32_t*, void*);
static gw_step_fb_fn g_step_fb = NULL;
static gw_reset_fn g_reset = NULL;

static int as_ptr(PyObject* o, void** out)
{
    const unsigned long long v = PyLong_AsUnsignedLongLong(o);
    if (v == (unsigned long long)-1 && PyErr_Occurred()) return -1;
    *out = (void*)(uintptr_t)v;
    return 0;
}

/* bind(addr_of_gw_step, addr_of_gw_pendulum_step, addr_of_gw_step_fb[, addr_of_gw_reset]) */
static PyObject* py_bind(PyObject* self, PyObject* const* args, Py_ssize_t n)
{
    void *a = NULL, *b = NULL, *c = NULL, *d = NULL;
    if (n != 3 && n != 4) { PyErr_SetString(PyExc_TypeError, "bind(gw_step, gw_pendulum_step, gw_step_fb[, gw_reset])"); return NULL; }
    if (as_ptr(args[0], &a) || as_ptr(args[1], &b) || as_ptr(args[2], &c) || (n == 4 && as_ptr(args[3], &d))) return NULL;
    g_step = (gw_step_fn)a;
    g_pend = (gw_pend_fn)b;
    g_step_fb = (gw_step_fb_fn)c;
    g_reset = (gw_reset_fn)d;
    Py_RETURN_NONE;
}

/* gw_episodes (include/gymwipe_amd.h), restated: this file includes nothing of the library's */
typedef struct { int32_t max_steps, on_done; int32_t* state_dev; int64_t* tally_dev; } gw_episodes_rec;
typedef int (*gw_autoreset_fn)(void*, int32_t, const int32_t*, const int32_t*, const gw_episodes_rec*, int32_t*, int32_t*, float*,
                               uint8_t*, uint8_t*, void*);
static gw_autoreset_fn g_autoreset = NULL;

/* bind_autoreset(addr_of_gw_rollout_autoreset): a call of its own, so that bind()'s arity stays */
static PyObject* py_bind_autoreset(PyObject* self, PyObject* const* args, Py_ssize_t n)
{
    void* a = NULL;
    if (n != 1) { PyErr_SetString(PyExc_TypeError, "bind_autoreset(gw_rollout_autoreset)"); return NULL; }
    if (as_ptr(args[0], &a)) return NULL;
    g_autoreset = (gw_autoreset_fn)a;
    Py_RETURN_NONE;
}

/* rollout_autoreset(env, steps, device, duration, max_steps, on_done, state, tally, obs_next, obs, reward, done, ended, stream)
 * -> rc; addresses and three ints in, the gw_episodes record built on the C stack */
static PyObject* py_autoreset(PyObject* self, PyObject* const* args, Py_ssize_t n)
{
    void* p[14];
    long v[3];
    if (n != 14 || !g_autoreset) {
        PyErr_SetString(PyExc_TypeError, "rollout_autoreset(env, steps, device, duration, max_steps, on_done, state, tally, obs_next, "
                                         "obs, reward, done, ended, stream) after bind_autoreset()");
        return NULL;
    }
    for (int i = 0; i < 14; ++i) {
        if (i == 1 || i == 4 || i == 5) {
            long* w = &v[i == 1 ? 0 : i - 3];
            *w = PyLong_AsLong(args[i]);
            if (*w == -1 && PyErr_Occurred()) return NULL;
            if (*w < INT32_MIN || *w > INT32_MAX) { PyErr_SetString(PyExc_OverflowError, "rollout_autoreset: int32 expected"); return NULL; }
        } else if (as_ptr(args[i], &p[i])) return NULL;
    }
    const gw_episodes_rec ep = {(int32_t)v[1], (int32_t)v[2], (int32_t*)p[6], (int64_t*)p[7]};
    const int rc = g_autoreset(p[0], (int32_t)v[0], (const int32_t*)p[2], (const int32_t*)p[3], &ep, (int32_t*)p[8], (int32_t*)p[9],
                               (float*)p[10], (uint8_t*)p[11], (uint8_t*)p[12], p[13]);
    return PyLong_FromLong(rc);
}

/* reset(env, mask, obs, stream) -> rc */
static PyObject* py_reset(PyObject* self, PyObject* const* args, Py_ssize_t n)
{
    void* p[4];
    if (n != 4 || !g_reset) { PyErr_SetString(PyExc_TypeError, "reset(env, mask, obs, stream) after bind() with gw_reset"); return NULL; }
    for (int i = 0; i < 4; ++i)
        if (as_ptr(args[i], &p[i])) return NULL;
    return PyLong_FromLong(g_reset(p[0], (const uint8_t*)p[1], (int32_t*)p[2], p[3]));
}

/* step_fb(env, device, duration, obs, reward, done, feedback_byte, stream) -> rc */
static PyObject* py_step_fb(PyObject* self, PyObject* const* args, Py_ssize_t n)
{
    void* p[8];
    if (n != 8 || !g_step_fb) { PyErr_SetString(PyExc_TypeError, "step_fb(env, device, duration, obs, reward, done, feedback_byte, stream) after bind()"); return NULL; }
    for (int i = 0; i < 8; ++i)
        if (as_ptr(args[i], &p[i])) return NULL;
    const int rc = g_step_fb(p[0], (const int32_t*)p[1], (const int32_t*)p[2], (int32_t*)p[3], (float*)p[4], (uint8_t*)p[5], (uint8_t*)p[6], p[7]);
    return PyLong_FromLong(rc);
}

/* step(env, device, duration, obs, reward, done, stream) -> rc; all arguments are addresses as Python ints */
static PyObject* py_step(PyObject* self, PyObject* const* args, Py_ssize_t n)
{
    void* p[7];
    if (n != 7 || !g_step) { PyErr_SetString(PyExc_TypeError, "step(env, device, duration, obs, reward, done, stream) after bind()"); return NULL; }
    for (int i = 0; i < 7; ++i)
        if (as_ptr(args[i], &p[i])) return NULL;
    const int rc = g_step(p[0], (const int32_t*)p[1], (const int32_t*)p[2], (int32_t*)p[3], (float*)p[4], (uint8_t*)p[5], p[6]);
    return PyLong_FromLong(rc);
}

/* pendulum_step(env, plant, device, duration, obs, reward, angle_deg, stream) -> rc */
static PyObject* py_pend(PyObject* self, PyObject* const* args, Py_ssize_t n)
{
    void* p[8];
    if (n != 8 || !g_pend) { PyErr_SetString(PyExc_TypeError, "pendulum_step(env, plant, device, duration, obs, reward, angle, stream) after bind()"); return NULL; }
    for (int i = 0; i < 8; ++i)
        if (as_ptr(args[i], &p[i])) return NULL;
    const int rc = g_pend(p[0], p[1], (const int32_t*)p[2], (const int32_t*)p[3], (int32_t*)p[4], (float*)p[5], (double*)p[6], p[7]);
    return PyLong_FromLong(rc);
}

/* ---- Stepper: env.step(action, out) of VecCounterTrafficEnv as one vectorcall ------------------------------------------------
 * Stepper(handle, device_index, seen, get_device, get_raw_stream, env, fallback, check, outputs_type)
 *   handle          address of the gw_env (the attribute `handle` is writable: env.close() zeroes it)
 *   seen            the env's identity cache {id(tensor): (weakref(tensor), data_ptr)} -- the SAME dict object
 *   get_device      torch._C._cuda_getDevice            get_raw_stream   torch._C._cuda_getCurrentRawStream
 *   env             receives `_last`                    fallback         the Python method (validates, fills the cache, raises)
 *   check           _native.check: turns a non-zero rc into the exception     outputs_type   StepOutputs (exact type)
 * A call takes the native route when `out` is a StepOutputs of this device, the current device is the env's and both action
 * tensors hit the cache; everything else is handed to `fallback` with the caller's arguments untouched.
 * References: `args` are the caller's for the whole call; everything read out of `action`, `seen` and `out` is borrowed and
 * used only between the two calls into torch (done first) and the launch -- no Python code runs in between; what is needed
 * after the launch (the result tuple, `_as_tuple`) is owned before env._last is assigned. */
typedef struct {
    PyObject_HEAD
    vectorcallfunc vc;
    unsigned long long handle;
    long dev_index;
    PyObject *seen, *get_device, *get_stream, *env, *fallback, *check, *out_type, *dev_index_obj;
    Py_ssize_t off_obs, off_reward, off_done, off_ptrs, off_tuple, off_dev;   /* StepOutputs' slots */
} Stepper;

static PyObject *s_device, *s_duration, *s_out, *s_last;

static int slot_offset(PyObject* type, const char* name, Py_ssize_t* off)
{
    PyObject* d = PyDict_GetItemString(((PyTypeObject*)type)->tp_dict, name);      /* borrowed */
    if (!d || Py_TYPE(d) != &PyMemberDescr_Type || ((PyMemberDescrObject*)d)->d_member->type != T_OBJECT_EX) {
        PyErr_Format(PyExc_TypeError, "Stepper: outputs_type has no slot %s", name);
        return -1;
    }
    *off = ((PyMemberDescrObject*)d)->d_member->offset;
    return 0;
}

/* address of a cached action tensor, or 0 */
static inline int cached_ptr(PyObject* seen, PyObject* t, void** out)
{
    PyObject* key = PyLong_FromVoidPtr(t);                    /* id(t) */
    if (!key) return -1;
    PyObject* hit = PyDict_GetItemWithError(seen, key);       /* borrowed */
    Py_DECREF(key);
    if (!hit) return PyErr_Occurred() ? -1 : 1;
    if (!PyTuple_CheckExact(hit) || PyTuple_GET_SIZE(hit) != 2) return 1;
    PyObject* ref = PyTuple_GET_ITEM(hit, 0);
    if (!PyWeakref_CheckRef(ref) || PyWeakref_GET_OBJECT(ref) != t) return 1;     /* `hit[0]() is t` */
    if (as_ptr(PyTuple_GET_ITEM(hit, 1), out)) return -1;
    return 0;
}

static PyObject* stepper_call(PyObject* self_, PyObject* const* args, size_t nargsf, PyObject* kwnames)
{
    Stepper* self = (Stepper*)self_;
    const Py_ssize_t nargs = PyVectorcall_NARGS(nargsf);
    const Py_ssize_t nkw = kwnames ? PyTuple_GET_SIZE(kwnames) : 0;
    PyObject *action = NULL, *out = NULL;
    if (nargs == 2 && nkw == 0) { action = args[0]; out = args[1]; }
    else if (nargs == 1 && nkw == 1) {                         /* step(action, out=...) */
        PyObject* k = PyTuple_GET_ITEM(kwnames, 0);
        if (k == s_out || (PyUnicode_CheckExact(k) && PyUnicode_Compare(k, s_out) == 0)) { action = args[0]; out = args[1]; }
    }
    if (!action || Py_TYPE(out) != (PyTypeObject*)self->out_type || !PyDict_CheckExact(action)) goto fallback;
    {
        /* the two calls into torch first: nothing borrowed is held across them */
        PyObject* cur = PyObject_CallNoArgs(self->get_device);
        if (!cur) return NULL;
        const long cur_dev = PyLong_AsLong(cur);
        Py_DECREF(cur);
        if (cur_dev == -1 && PyErr_Occurred()) return NULL;
        if (cur_dev != self->dev_index) goto fallback;
        PyObject* so = PyObject_CallOneArg(self->get_stream, self->dev_index_obj);
        if (!so) return NULL;
        void* stream = NULL;
        const int bad = as_ptr(so, &stream);
        Py_DECREF(so);
        if (bad) return NULL;

        PyObject* o_dev = *(PyObject**)((char*)out + self->off_dev);
        PyObject* o_ptrs = *(PyObject**)((char*)out + self->off_ptrs);
        PyObject* o_tuple = *(PyObject**)((char*)out + self->off_tuple);
        PyObject* o_obs = *(PyObject**)((char*)out + self->off_obs);
        PyObject* o_rew = *(PyObject**)((char*)out + self->off_reward);
        PyObject* o_done = *(PyObject**)((char*)out + self->off_done);
        if (!o_dev || !o_ptrs || !o_tuple || !o_obs || !o_rew || !o_done || !PyLong_CheckExact(o_dev) ||
            !PyTuple_CheckExact(o_ptrs) || PyTuple_GET_SIZE(o_ptrs) != 4)
            goto fallback;
        const long odev = PyLong_AsLong(o_dev);
        if (odev == -1 && PyErr_Occurred()) return NULL;
        if (odev != self->dev_index) goto fallback;            /* (the Python method raises the ValueError) */
        PyObject* dev = PyDict_GetItemWithError(action, s_device);
        if (!dev) { if (PyErr_Occurred()) return NULL; goto fallback; }
        PyObject* dur = PyDict_GetItemWithError(action, s_duration);
        if (!dur) { if (PyErr_Occurred()) return NULL; goto fallback; }
        void *p_dev = NULL, *p_dur = NULL, *p[4];
        int miss = cached_ptr(self->seen, dev, &p_dev);
        if (miss < 0) return NULL;
        if (miss) goto fallback;
        miss = cached_ptr(self->seen, dur, &p_dur);
        if (miss < 0) return NULL;
        if (miss) goto fallback;
        for (int i = 0; i < 4; ++i)
            if (as_ptr(PyTuple_GET_ITEM(o_ptrs, i), &p[i])) return NULL;
        if (!g_step || !g_step_fb) goto fallback;

        void* h = (void*)(uintptr_t)self->handle;
        const int rc = p[3] ? g_step_fb(h, (const int32_t*)p_dev, (const int32_t*)p_dur, (int32_t*)p[0], (float*)p[1], (uint8_t*)p[2], (uint8_t*)p[3], stream)
                            : g_step(h, (const int32_t*)p_dev, (const int32_t*)p_dur, (int32_t*)p[0], (float*)p[1], (uint8_t*)p[2], stream);
        if (rc) {                                              /* _native.check(rc) raises NativeError with the library's message */
            PyObject* rco = PyLong_FromLong(rc);
            if (!rco) return NULL;
            PyObject* r = PyObject_CallOneArg(self->check, rco);
            Py_DECREF(rco);
            if (!r) return NULL;
            Py_DECREF(r);
            PyErr_Format(PyExc_RuntimeError, "gymwipe_amd native error %d", rc);
            return NULL;
        }
        PyObject* info = PyDict_New();
        if (!info) return NULL;
        PyObject* res = PyTuple_New(4);
        if (!res) { Py_DECREF(info); return NULL; }
        Py_INCREF(o_obs); Py_INCREF(o_rew); Py_INCREF(o_done);
        PyTuple_SET_ITEM(res, 0, o_obs); PyTuple_SET_ITEM(res, 1, o_rew); PyTuple_SET_ITEM(res, 2, o_done); PyTuple_SET_ITEM(res, 3, info);
        Py_INCREF(o_tuple);
        const int sr = PyObject_SetAttr(self->env, s_last, o_tuple);
        Py_DECREF(o_tuple);
        if (sr) { Py_DECREF(res); return NULL; }
        return res;
    }
fallback:
    return PyObject_Vectorcall(self->fallback, args, nargsf & ~PY_VECTORCALL_ARGUMENTS_OFFSET, kwnames);
}

static int stepper_traverse(PyObject* o, visitproc visit, void* arg)
{
    Stepper* s = (Stepper*)o;
    Py_VISIT(s->seen); Py_VISIT(s->get_device); Py_VISIT(s->get_stream); Py_VISIT(s->env); Py_VISIT(s->fallback);
    Py_VISIT(s->check); Py_VISIT(s->out_type); Py_VISIT(s->dev_index_obj);
    return 0;
}

static int stepper_clear(PyObject* o)
{
    Stepper* s = (Stepper*)o;
    Py_CLEAR(s->seen); Py_CLEAR(s->get_device); Py_CLEAR(s->get_stream); Py_CLEAR(s->env); Py_CLEAR(s->fallback);
    Py_CLEAR(s->check); Py_CLEAR(s->out_type); Py_CLEAR(s->dev_index_obj);
    return 0;
}

static void stepper_dealloc(PyObject* o)
{
    PyObject_GC_UnTrack(o);
    stepper_clear(o);
    Py_TYPE(o)->tp_free(o);
}

static PyObject* stepper_new(PyTypeObject* type, PyObject* args, PyObject* kw)
{
    PyObject *h, *idx, *seen, *gd, *gs, *env, *fb, *chk, *ot;
    if (kw && PyDict_GET_SIZE(kw)) { PyErr_SetString(PyExc_TypeError, "Stepper() takes no keyword arguments"); return NULL; }
    if (!PyArg_ParseTuple(args, "O!O!O!OOOOOO!:Stepper", &PyLong_Type, &h, &PyLong_Type, &idx, &PyDict_Type, &seen, &gd, &gs, &env, &fb,
                          &chk, &PyType_Type, &ot))
        return NULL;
    if (!PyCallable_Check(gd) || !PyCallable_Check(gs) || !PyCallable_Check(fb) || !PyCallable_Check(chk)) {
        PyErr_SetString(PyExc_TypeError, "Stepper: get_device, get_raw_stream, fallback and check must be callable");
        return NULL;
    }
    const unsigned long long hv = PyLong_AsUnsignedLongLong(h);
    if (hv == (unsigned long long)-1 && PyErr_Occurred()) return NULL;
    const long di = PyLong_AsLong(idx);
    if (di == -1 && PyErr_Occurred()) return NULL;
    Py_ssize_t off[6];
    static const char* const names[6] = {"obs", "reward", "done", "_ptrs", "_as_tuple", "_dev"};
    for (int i = 0; i < 6; ++i)
        if (slot_offset(ot, names[i], &off[i])) return NULL;
    Stepper* s = (Stepper*)type->tp_alloc(type, 0);
    if (!s) return NULL;
    s->vc = stepper_call;
    s->handle = hv;
    s->dev_index = di;
    s->off_obs = off[0]; s->off_reward = off[1]; s->off_done = off[2]; s->off_ptrs = off[3]; s->off_tuple = off[4]; s->off_dev = off[5];
    Py_INCREF(seen); s->seen = seen;
    Py_INCREF(gd); s->get_device = gd;
    Py_INCREF(gs); s->get_stream = gs;
    Py_INCREF(env); s->env = env;
    Py_INCREF(fb); s->fallback = fb;
    Py_INCREF(chk); s->check = chk;
    Py_INCREF(ot); s->out_type = ot;
    Py_INCREF(idx); s->dev_index_obj = idx;
    return (PyObject*)s;
}

static PyMemberDef stepper_members[] = {
    {"handle", T_ULONGLONG, offsetof(Stepper, handle), 0, "address of the gw_env; 0 after env.close()"},
    {"fallback", T_OBJECT, offsetof(Stepper, fallback), READONLY, "the Python method every other case goes to"},
    {NULL}};

static PyTypeObject StepperType = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "_gw_fast.Stepper",
    .tp_basicsize = sizeof(Stepper),
    .tp_dealloc = stepper_dealloc,
    .tp_vectorcall_offset = offsetof(Stepper, vc),
    .tp_call = PyVectorcall_Call,
    .tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_HAVE_GC | Py_TPFLAGS_HAVE_VECTORCALL,       /* no Py_TPFLAGS_BASETYPE */
    .tp_doc = "env.step(action, out) of VecCounterTrafficEnv as one native call",
    .tp_traverse = stepper_traverse,
    .tp_clear = stepper_clear,
    .tp_members = stepper_members,
    .tp_new = stepper_new,
};

static PyMethodDef methods[] = {
    {"bind", (PyCFunction)(void (*)(void))py_bind, METH_FASTCALL, "bind(gw_step address, gw_pendulum_step address, gw_step_fb address[, gw_reset address])"},
    {"bind_autoreset", (PyCFunction)(void (*)(void))py_bind_autoreset, METH_FASTCALL, "bind_autoreset(gw_rollout_autoreset address)"},
    {"rollout_autoreset", (PyCFunction)(void (*)(void))py_autoreset, METH_FASTCALL, "gw_rollout_autoreset with addresses and ints"},
    {"reset", (PyCFunction)(void (*)(void))py_reset, METH_FASTCALL, "gw_reset with addresses as ints"},
    {"step", (PyCFunction)(void (*)(void))py_step, METH_FASTCALL, "gw_step with addresses as ints"},
    {"step_fb", (PyCFunction)(void (*)(void))py_step_fb, METH_FASTCALL, "gw_step_fb with addresses as ints"},
    {"pendulum_step", (PyCFunction)(void (*)(void))py_pend, METH_FASTCALL, "gw_pendulum_step with addresses as ints"},
    {NULL, NULL, 0, NULL}};

static struct PyModuleDef moddef = {PyModuleDef_HEAD_INIT, "_gw_fast", "fast-call shim for the per-step C-ABI entry points", -1, methods};

PyMODINIT_FUNC PyInit__gw_fast(void)
{
    if (PyType_Ready(&StepperType) < 0) return NULL;
    if (!(s_device = PyUnicode_InternFromString("device")) || !(s_duration = PyUnicode_InternFromString("duration")) ||
        !(s_out = PyUnicode_InternFromString("out")) || !(s_last = PyUnicode_InternFromString("_last")))
        return NULL;
    PyObject* m = PyModule_Create(&moddef);
    if (!m) return NULL;
    Py_INCREF(&StepperType);
    if (PyModule_AddObject(m, "Stepper", (PyObject*)&StepperType) < 0) { Py_DECREF(&StepperType); Py_DECREF(m); return NULL; }
    return m;
}
