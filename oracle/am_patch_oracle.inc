/* am_patch_oracle.inc -- CPU restatement of Backend.getPatch() (included by am_oracle.c).
 *
 * TEST INFRASTRUCTURE ONLY. Restates, sequentially:
 *   getPatch                              new.js:2052-2060
 *   documentPatch                         new.js:1604-1635
 *   updatePatchProperty (whole document)  new.js:884-1040 (newBlock == null, oldSuccNum = succNum)
 *   appendEdit / appendUpdate             new.js:747-823
 *   emptyObjectPatch                      new.js:726-732
 *   decodeValue                           columnar.js:300-329
 * and emits the patch as JSON (Uint8Array values as {"__bytes": hex}, as the fixture generator
 * does). Pinned by the getPatch results in tests/golden/docs.json (produced by the reference).
 */

/* ---- patch tree ---- */
typedef struct pnode pnode;
enum { PV_NONE = 0, PV_OP, PV_COUNTER, PV_CHILD };
typedef struct { int kind; const op_t *op; int64_t counter; pnode *child; } pval;
typedef struct { int64_t ctr; int64_t actor; pval v; } pentry;
typedef struct { const uint8_t *key; uint32_t keyn; pentry *e; size_t n, cap; } pprop;
enum { ED_INSERT = 0, ED_MULTI, ED_UPDATE, ED_REMOVE };
typedef struct {
  int action;
  int64_t index, count;
  int64_t elem_ctr, elem_actor;  /* elemId */
  int64_t op_ctr, op_actor;      /* opId */
  pval value;
  pval *values; size_t nvalues, capvalues;
  int has_dt; int dt_num; const char *dt_str; /* multi-insert datatype */
} pedit;
struct pnode {
  int64_t obj_ctr, obj_actor; /* -1 = _root */
  const char *type;           /* map / list / text / table */
  pprop *props; size_t nprops, capprops;
  pedit *edits; size_t nedits, capedits;
  pnode *next;                /* registry */
};

#define GROW(c, arr, n, cap, T)                              \
  do {                                                        \
    if ((n) == (cap)) {                                       \
      size_t nc_ = (cap) ? 2 * (cap) : 4;                     \
      T *na_ = (T *)amalloc((c), sizeof(T) * nc_);            \
      if (n) { memcpy(na_, (arr), sizeof(T) * (n)); }         \
      (arr) = na_;                                            \
      (cap) = nc_;                                            \
    }                                                         \
  } while (0)

static const char *ACTION_OBJ_TYPE[8] = {"map", NULL, "list", NULL, "text", NULL, "table", NULL};

/* decodeValue classification: JS typeof of the value and its datatype annotation */
enum { TY_OBJECT = 0, TY_BOOLEAN, TY_STRING, TY_NUMBER };
typedef struct { int ty; int has_dt; int dt_num; const char *dt_str; } vclass;
static vclass value_class(ctx_t *c, const op_t *op) {
  vclass r = {TY_OBJECT, 0, 0, NULL};
  const int64_t tag = op->val_len.null ? 0 : op->val_len.v;
  if (tag == 0) return r;                       /* null */
  if (tag == 1 || tag == 2) { r.ty = TY_BOOLEAN; return r; }
  switch (tag % 16) {
    case 6: r.ty = TY_STRING; return r;
    case 3: r.ty = TY_NUMBER; r.has_dt = 1; r.dt_str = "uint"; return r;
    case 4: r.ty = TY_NUMBER; r.has_dt = 1; r.dt_str = "int"; return r;
    case 5:
      if (op->val_raw_n != 8) fail(c, "Invalid length for floating point number: %u", op->val_raw_n);
      r.ty = TY_NUMBER; r.has_dt = 1; r.dt_str = "float64"; return r;
    case 8: r.ty = TY_NUMBER; r.has_dt = 1; r.dt_str = "counter"; return r;
    case 9: r.ty = TY_NUMBER; r.has_dt = 1; r.dt_str = "timestamp"; return r;
    default: r.ty = TY_OBJECT; r.has_dt = 1; r.dt_num = (int)(tag % 16); return r;  /* bytes / unknown */
  }
}
/* datatype annotations are equal (=== on strings / numbers; an absent one is undefined) */
static int dt_eq(int ha, int na, const char *sa, int hb, int nb, const char *sb) {
  if (ha != hb) return 0;
  if (!ha) return 1;
  if (sa || sb) return sa && sb && strcmp(sa, sb) == 0;
  return na == nb;
}
/* datatype is truthy (0 is falsy) */
static int dt_truthy(vclass v) { return v.has_dt && (v.dt_str || v.dt_num != 0); }

static int64_t value_int(ctx_t *c, const op_t *op) {
  rd_t d = {op->val_raw, op->val_raw_n, 0};
  const int64_t tag = op->val_len.null ? 0 : op->val_len.v;
  if (tag % 16 == 3) return rd_u53(c, &d);
  return rd_i53(c, &d);
}
/* counterState.value += decodeValue(...).value (new.js:958): null and false add 0, true adds 1 */
static int64_t inc_amount(ctx_t *c, const op_t *op) {
  const int64_t tag = op->val_len.null ? 0 : op->val_len.v;
  if (tag == 0 || tag == 1) return 0;
  if (tag == 2) return 1;
  if (value_class(c, op).ty != TY_NUMBER) unsupported(c, "non-numeric counter increment");
  return value_int(c, op);
}

/* ---- JSON output ---- */
static void js_raw(ctx_t *c, bbuf *o, const char *s) { bb_raw(c, o, (const uint8_t *)s, strlen(s)); }
static void js_fmt(ctx_t *c, bbuf *o, const char *f, ...) {
  char b[96];
  va_list ap;
  va_start(ap, f);
  vsnprintf(b, sizeof b, f, ap);
  va_end(ap);
  js_raw(c, o, b);
}
static void js_str(ctx_t *c, bbuf *o, const uint8_t *s, size_t n) {
  bb_byte(c, o, '"');
  size_t i = 0;
  while (i < n) {
    size_t st = i;
    uint32_t cp = utf8_next(s, n, &i);
    if (cp == '"') js_raw(c, o, "\\\"");
    else if (cp == '\\') js_raw(c, o, "\\\\");
    else if (cp < 0x20) js_fmt(c, o, "\\u%04x", cp);
    else if (cp == 0xfffd && !(i - st == 3 && s[st] == 0xef)) js_raw(c, o, "\xef\xbf\xbd");
    else bb_raw(c, o, s + st, i - st);
  }
  bb_byte(c, o, '"');
}
static void js_hex(ctx_t *c, bbuf *o, const uint8_t *p, size_t n) {
  static const char *H = "0123456789abcdef";
  bb_byte(c, o, '"');
  for (size_t i = 0; i < n; i++) { bb_byte(c, o, H[p[i] >> 4]); bb_byte(c, o, H[p[i] & 15]); }
  bb_byte(c, o, '"');
}
static void js_opid(ctx_t *c, bbuf *o, const docst_t *st, int64_t ctr, int64_t actor) {
  char a[130];
  hex_actor(st->actors[actor], st->actor_lens[actor], a);
  js_fmt(c, o, "\"%lld@", (long long)ctr);
  js_raw(c, o, a);
  bb_byte(c, o, '"');
}
/* the JS primitive of decodeValue(...).value */
static void js_prim(ctx_t *c, bbuf *o, const op_t *op) {
  const int64_t tag = op->val_len.null ? 0 : op->val_len.v;
  if (tag == 0) { js_raw(c, o, "null"); return; }
  if (tag == 1) { js_raw(c, o, "false"); return; }
  if (tag == 2) { js_raw(c, o, "true"); return; }
  switch (tag % 16) {
    case 6: js_str(c, o, op->val_raw, op->val_raw_n); return;
    case 3: case 4: case 8: case 9: js_fmt(c, o, "%lld", (long long)value_int(c, op)); return;
    case 5: {
      double dv;
      memcpy(&dv, op->val_raw, 8); /* little-endian host */
      if (dv != dv || dv == 1.0 / 0.0 || dv == -1.0 / 0.0) js_raw(c, o, "null"); /* JSON.stringify */
      else js_fmt(c, o, "%.17g", dv);
      return;
    }
    default: js_raw(c, o, "{\"__bytes\":"); js_hex(c, o, op->val_raw, op->val_raw_n); bb_byte(c, o, '}'); return;
  }
}
static void js_dt(ctx_t *c, bbuf *o, int has, int num, const char *s) {
  if (!has) return;
  if (s) { js_raw(c, o, ",\"datatype\":\""); js_raw(c, o, s); bb_byte(c, o, '"'); }
  else js_fmt(c, o, ",\"datatype\":%d", num);
}
static void js_node(ctx_t *c, bbuf *o, const docst_t *st, const pnode *nd);
static void js_val(ctx_t *c, bbuf *o, const docst_t *st, const pval *v) {
  if (v->kind == PV_CHILD) { js_node(c, o, st, v->child); return; }
  if (v->kind == PV_COUNTER) { js_fmt(c, o, "{\"type\":\"value\",\"datatype\":\"counter\",\"value\":%lld}", (long long)v->counter); return; }
  vclass k = value_class(c, v->op);
  js_raw(c, o, "{\"type\":\"value\",\"value\":");
  js_prim(c, o, v->op);
  js_dt(c, o, k.has_dt, k.dt_num, k.dt_str);
  bb_byte(c, o, '}');
}
static void js_node(ctx_t *c, bbuf *o, const docst_t *st, const pnode *nd) {
  js_raw(c, o, "{\"objectId\":");
  if (nd->obj_actor < 0) js_raw(c, o, "\"_root\"");
  else js_opid(c, o, st, nd->obj_ctr, nd->obj_actor);
  js_raw(c, o, ",\"type\":\"");
  js_raw(c, o, nd->type);
  bb_byte(c, o, '"');
  const int is_list = strcmp(nd->type, "list") == 0 || strcmp(nd->type, "text") == 0;
  if (is_list) {
    js_raw(c, o, ",\"edits\":[");
    for (size_t i = 0; i < nd->nedits; i++) {
      const pedit *e = &nd->edits[i];
      if (i) bb_byte(c, o, ',');
      if (e->action == ED_REMOVE) { js_fmt(c, o, "{\"action\":\"remove\",\"index\":%lld,\"count\":%lld}", (long long)e->index, (long long)e->count); continue; }
      if (e->action == ED_UPDATE) {
        js_fmt(c, o, "{\"action\":\"update\",\"index\":%lld,\"opId\":", (long long)e->index);
        js_opid(c, o, st, e->op_ctr, e->op_actor);
        js_raw(c, o, ",\"value\":");
        js_val(c, o, st, &e->value);
        bb_byte(c, o, '}');
        continue;
      }
      js_fmt(c, o, "{\"action\":\"%s\",\"index\":%lld,\"elemId\":", e->action == ED_MULTI ? "multi-insert" : "insert", (long long)e->index);
      js_opid(c, o, st, e->elem_ctr, e->elem_actor);
      if (e->action == ED_INSERT) {
        js_raw(c, o, ",\"opId\":");
        js_opid(c, o, st, e->op_ctr, e->op_actor);
        js_raw(c, o, ",\"value\":");
        js_val(c, o, st, &e->value);
      } else {
        js_dt(c, o, e->has_dt, e->dt_num, e->dt_str);
        js_raw(c, o, ",\"values\":[");
        for (size_t k = 0; k < e->nvalues; k++) {
          if (k) bb_byte(c, o, ',');
          if (e->values[k].kind == PV_COUNTER) js_fmt(c, o, "%lld", (long long)e->values[k].counter);
          else js_prim(c, o, e->values[k].op);
        }
        bb_byte(c, o, ']');
      }
      bb_byte(c, o, '}');
    }
    bb_byte(c, o, ']');
  } else {
    js_raw(c, o, ",\"props\":{");
    for (size_t i = 0; i < nd->nprops; i++) {
      const pprop *p = &nd->props[i];
      if (i) bb_byte(c, o, ',');
      js_str(c, o, p->key, p->keyn);
      js_raw(c, o, ":{");
      for (size_t k = 0; k < p->n; k++) {
        if (k) bb_byte(c, o, ',');
        js_opid(c, o, st, p->e[k].ctr, p->e[k].actor);
        bb_byte(c, o, ':');
        js_val(c, o, st, &p->e[k].v);
      }
      bb_byte(c, o, '}');
    }
    bb_byte(c, o, '}');
  }
  bb_byte(c, o, '}');
}

/* ---- patch construction ---- */
typedef struct { pnode *head; } preg;
static pnode *reg_find(preg *r, int64_t ctr, int64_t actor) {
  for (pnode *n = r->head; n; n = n->next)
    if (n->obj_ctr == ctr && n->obj_actor == actor) return n;
  return NULL;
}
static pnode *reg_new(ctx_t *c, preg *r, int64_t ctr, int64_t actor, const char *type) {
  pnode *n = (pnode *)amalloc(c, sizeof(pnode));
  memset(n, 0, sizeof *n);
  n->obj_ctr = ctr;
  n->obj_actor = actor;
  n->type = type;
  n->next = r->head;
  r->head = n;
  return n;
}
/* objectMeta: the type of each object created by a make op (only the type is observable here) */
typedef struct omet { int64_t ctr, actor; const char *type; struct omet *next; } omet;

/* the value's JS primitive typeof for the multi-insert check (counters are numbers) */
static int pval_ty(ctx_t *c, const pval *v) { return v->kind == PV_COUNTER ? TY_NUMBER : value_class(c, v->op).ty; }
static vclass pval_class(ctx_t *c, const pval *v) {
  if (v->kind == PV_COUNTER) { vclass k = {TY_NUMBER, 1, 0, "counter"}; return k; }
  return value_class(c, v->op);
}

/* appendEdit (new.js:747-782) */
static void append_edit(ctx_t *c, pnode *p, pedit ne) {
  if (p->nedits == 0) { GROW(c, p->edits, p->nedits, p->capedits, pedit); p->edits[p->nedits++] = ne; return; }
  pedit *last = &p->edits[p->nedits - 1];
  if (last->action == ED_INSERT && ne.action == ED_INSERT && last->index == ne.index - 1 &&
      last->value.kind != PV_CHILD && ne.value.kind != PV_CHILD &&
      last->elem_ctr == last->op_ctr && last->elem_actor == last->op_actor &&
      ne.elem_ctr == ne.op_ctr && ne.elem_actor == ne.op_actor &&
      last->elem_actor == ne.elem_actor && last->elem_ctr + 1 == ne.elem_ctr) {
    vclass a = pval_class(c, &last->value), b = pval_class(c, &ne.value);
    if (dt_eq(a.has_dt, a.dt_num, a.dt_str, b.has_dt, b.dt_num, b.dt_str) && a.ty == b.ty) {
      last->action = ED_MULTI;
      last->has_dt = 0;
      if (dt_truthy(b)) { last->has_dt = 1; last->dt_num = b.dt_num; last->dt_str = b.dt_str; }
      last->nvalues = 0;
      GROW(c, last->values, last->nvalues, last->capvalues, pval);
      last->values[last->nvalues++] = last->value;
      GROW(c, last->values, last->nvalues, last->capvalues, pval);
      last->values[last->nvalues++] = ne.value;
      return;
    }
  }
  if (last->action == ED_MULTI && ne.action == ED_INSERT && last->index + (int64_t)last->nvalues == ne.index &&
      ne.value.kind != PV_CHILD && ne.elem_ctr == ne.op_ctr && ne.elem_actor == ne.op_actor &&
      last->elem_actor == ne.elem_actor && last->elem_ctr + (int64_t)last->nvalues == ne.elem_ctr) {
    vclass b = pval_class(c, &ne.value);
    if (dt_eq(last->has_dt, last->dt_num, last->dt_str, b.has_dt, b.dt_num, b.dt_str) &&
        pval_ty(c, &last->values[0]) == b.ty) {
      GROW(c, last->values, last->nvalues, last->capvalues, pval);
      last->values[last->nvalues++] = ne.value;
      return;
    }
  }
  if (last->action == ED_REMOVE && ne.action == ED_REMOVE && last->index == ne.index) { last->count += ne.count; return; }
  GROW(c, p->edits, p->nedits, p->capedits, pedit);
  p->edits[p->nedits++] = ne;
}

/* appendUpdate (new.js:797-823) */
static void append_update(ctx_t *c, pnode *p, int64_t index, int64_t ec, int64_t ea, int64_t oc, int64_t oa, pval v, int first) {
  int insert = 0;
  if (first) {
    while (!insert && p->nedits > 0) {
      pedit *last = &p->edits[p->nedits - 1];
      if ((last->action == ED_INSERT || last->action == ED_UPDATE) && last->index == index) {
        insert = last->action == ED_INSERT;
        p->nedits--;
      } else if (last->action == ED_MULTI && last->index + (int64_t)last->nvalues - 1 == index) {
        last->nvalues--;
        insert = 1;
      } else break;
    }
  }
  pedit e;
  memset(&e, 0, sizeof e);
  e.index = index;
  e.op_ctr = oc; e.op_actor = oa;
  e.value = v;
  if (insert) { e.action = ED_INSERT; e.elem_ctr = ec; e.elem_actor = ea; }
  else e.action = ED_UPDATE;
  append_edit(c, p, e);
}

/* per-key state (propState[elemId], new.js:910-912) */
typedef struct { int64_t succ_ctr, succ_actor; int state; } csucc;            /* counterStates entry */
typedef struct { int64_t op_ctr, op_actor, value; int nleft; } cstate;          /* counterState */
typedef struct {
  int active, has_child, action;  /* action: 0 none, 1 insert, 2 update, 3 remove */
  cstate *cs; size_t ncs, capcs;
  csucc *map; size_t nmap, capmap;
  int *done; /* per map entry: succ already consumed */
} pstate;

/* documentPatch (new.js:1604-1635) over the decoded document; returns the root patch node */
static pnode *document_patch(ctx_t *c, const docst_t *st, int64_t *max_op) {
  preg reg = {NULL};
  omet *meta = NULL;
  pnode *root = reg_new(c, &reg, -1, -1, "map");
  int64_t last_oa = -2, last_oc = -2, obj_ctr = -1, obj_actor = -1;
  int elem_visible = 0;
  int64_t list_index = 0;
  const char *obj_type = "map";
  /* key group tracking: ops of one key / element are adjacent in document order */
  const uint8_t *gkey = NULL; uint32_t gkeyn = 0; int64_t gec = -1, gea = -1; int gstr = -1;
  pstate ps;
  memset(&ps, 0, sizeof ps);
  *max_op = 0;
  for (size_t i = 0; i < st->nops; i++) {
    const op_t *op = &st->ops[i];
    const int64_t oa = op->obj_actor.null ? -1 : op->obj_actor.v, oc = op->obj_ctr.null ? -1 : op->obj_ctr.v;
    if (oa != last_oa || oc != last_oc) {
      obj_ctr = oc; obj_actor = oa;
      last_oa = oa; last_oc = oc;
      list_index = 0;
      elem_visible = 0;
      gstr = -1;
      obj_type = "map";
      if (oa >= 0) {
        obj_type = NULL;
        for (omet *m = meta; m; m = m->next) if (m->ctr == oc && m->actor == oa) obj_type = m->type;
        if (!obj_type) unsupported(c, "object without a make operation");
      }
    }
    const uint32_t nsucc = op->nsucc;
    if (op->insert && elem_visible) { elem_visible = 0; list_index++; }
    if (nsucc == 0) elem_visible = 1;
    if (op->id_ctr.v > *max_op) *max_op = op->id_ctr.v;
    for (uint32_t k = 0; k < nsucc; k++) if (op->succ_ctr[k].v > *max_op) *max_op = op->succ_ctr[k].v;

    /* ---- updatePatchProperty(patches, null, objectId, op, docState, propState, listIndex, succNum) ---- */
    const int64_t action = op->action.v;
    const int64_t id_ctr = op->id_ctr.v, id_actor = op->id_actor.v;
    const int has_key = !op->key_str.null && op->key_str.n > 0; /* op[keyStrIdx] is truthy */
    const int64_t ec = op->insert ? id_ctr : op->key_ctr.v, ea = op->insert ? id_actor : op->key_actor.v;
    if (action >= 0 && action < 8 && action % 2 == 0) {
      int known = 0;
      for (omet *m = meta; m; m = m->next) if (m->ctr == id_ctr && m->actor == id_actor) known = 1;
      if (!known) {
        omet *m = (omet *)amalloc(c, sizeof(omet));
        m->ctr = id_ctr; m->actor = id_actor; m->type = ACTION_OBJ_TYPE[action]; m->next = meta; meta = m;
      }
    }
    /* propState[elemId] -- a new group starts when the key / element changes */
    int same = 0;
    if (has_key) same = gstr == 1 && gkeyn == op->key_str.n && memcmp(gkey, op->key_str.p, gkeyn) == 0;
    else same = gstr == 0 && gec == ec && gea == ea;
    const int first_op = !same;
    if (!same) {
      memset(&ps, 0, sizeof ps);
      gstr = has_key;
      gkey = op->key_str.p; gkeyn = op->key_str.n; gec = ec; gea = ea;
    }
    const int overwritten = nsucc > 0;
    if (!overwritten) ps.has_child = ps.has_child || (action % 2) == 0;

    pval pv;
    memset(&pv, 0, sizeof pv);
    int64_t pk_ctr = 0, pk_actor = 0;
    const int64_t tag = op->val_len.null ? 0 : op->val_len.v;
    if (overwritten && action == 1 && (tag & 0x0f) == 8) {
      /* the set operation that creates a counter: all successors must turn out to be increments */
      GROW(c, ps.cs, ps.ncs, ps.capcs, cstate);
      cstate *cs = &ps.cs[ps.ncs++];
      cs->op_ctr = id_ctr; cs->op_actor = id_actor; cs->value = value_int(c, op); cs->nleft = 0;
      for (uint32_t k = 0; k < nsucc; k++) {
        /* counterStates[succOp] = counterState; counterState.succs[succOp] = true */
        size_t q = 0;
        while (q < ps.nmap && !(ps.map[q].succ_ctr == op->succ_ctr[k].v && ps.map[q].succ_actor == op->succ_actor[k].v)) q++;
        if (q == ps.nmap) { GROW(c, ps.map, ps.nmap, ps.capmap, csucc); ps.nmap++; }
        ps.map[q].succ_ctr = op->succ_ctr[k].v; ps.map[q].succ_actor = op->succ_actor[k].v; ps.map[q].state = (int)(ps.ncs - 1);
        int dup = 0;
        for (uint32_t j = 0; j < k; j++) if (op->succ_ctr[j].v == op->succ_ctr[k].v && op->succ_actor[j].v == op->succ_actor[k].v) dup = 1;
        if (!dup) cs->nleft++;
      }
    } else if (action == 5) {
      size_t q = 0;
      while (q < ps.nmap && !(ps.map[q].succ_ctr == id_ctr && ps.map[q].succ_actor == id_actor)) q++;
      if (q == ps.nmap) {
        char a[130];
        hex_actor(st->actors[id_actor], st->actor_lens[id_actor], a);
        fail(c, "increment operation %lld@%s for unknown counter", (long long)id_ctr, a);
      }
      cstate *cs = &ps.cs[ps.map[q].state];
      cs->value += inc_amount(c, op);
      /* delete counterState.succs[opId]: op ids are unique, so each successor is consumed once */
      cs->nleft--;
      if (cs->nleft == 0) {
        pv.kind = PV_COUNTER; pv.counter = cs->value;
        pk_ctr = cs->op_ctr; pk_actor = cs->op_actor;
      }
    } else if (!overwritten) {
      if (action == 1) { pv.kind = PV_OP; pv.op = op; pk_ctr = id_ctr; pk_actor = id_actor; }
      else if (action >= 0 && action < 8 && action % 2 == 0) {
        pnode *ch = reg_find(&reg, id_ctr, id_actor);
        if (!ch) ch = reg_new(c, &reg, id_ctr, id_actor, ACTION_OBJ_TYPE[action]);
        pv.kind = PV_CHILD; pv.child = ch; pk_ctr = id_ctr; pk_actor = id_actor;
      }
    }
    pnode *patch = reg_find(&reg, obj_ctr, obj_actor);
    if (!patch) patch = reg_new(c, &reg, obj_ctr, obj_actor, obj_type);
    if (!has_key) {
      if (pv.kind) {
        if (!ps.action) {
          ps.action = 1;
          pedit e;
          memset(&e, 0, sizeof e);
          e.action = ED_INSERT; e.index = list_index; e.elem_ctr = ec; e.elem_actor = ea;
          e.op_ctr = pk_ctr; e.op_actor = pk_actor; e.value = pv;
          append_edit(c, patch, e);
        } else if (ps.action == 3) {
          pedit *last = patch->nedits ? &patch->edits[patch->nedits - 1] : NULL;
          if (!last || last->action != ED_REMOVE) fail(c, "last edit has unexpected type");
          if (last->count > 1) last->count--; else patch->nedits--;
          ps.action = 2;
          append_update(c, patch, list_index, ec, ea, pk_ctr, pk_actor, pv, 1);
        } else {
          append_update(c, patch, list_index, ec, ea, pk_ctr, pk_actor, pv, 0);
        }
      } else if (nsucc == 0 && !ps.action) {
        ps.action = 3;
        pedit e;
        memset(&e, 0, sizeof e);
        e.action = ED_REMOVE; e.index = list_index; e.count = 1;
        append_edit(c, patch, e);
      }
    } else if (pv.kind) {
      pprop *pp = NULL;
      for (size_t k = 0; k < patch->nprops; k++)
        if (patch->props[k].keyn == op->key_str.n && memcmp(patch->props[k].key, op->key_str.p, op->key_str.n) == 0) pp = &patch->props[k];
      if (!pp) {
        GROW(c, patch->props, patch->nprops, patch->capprops, pprop);
        pp = &patch->props[patch->nprops++];
        memset(pp, 0, sizeof *pp);
        pp->key = op->key_str.p; pp->keyn = op->key_str.n;
      } else if (first_op) {
        pp->n = 0;
      }
      size_t k = 0;
      while (k < pp->n && !(pp->e[k].ctr == pk_ctr && pp->e[k].actor == pk_actor)) k++;
      if (k == pp->n) { GROW(c, pp->e, pp->n, pp->cap, pentry); pp->n++; }
      pp->e[k].ctr = pk_ctr; pp->e[k].actor = pk_actor; pp->e[k].v = pv;
    }
  }
  return root;
}

/* Backend.getPatch(doc) as JSON (malloc'd, NUL-terminated). Returns NULL on error. */
char *oc_doc_patch(const oc_doc *doc, char *err, size_t errcap) {
  CTX_BEGIN(c) { set_err(&c, err, errcap); afree_all(&c); return NULL; }
  docst_t st;
  load_state(&c, doc, &st);
  int64_t mx = 0;
  pnode *root = document_patch(&c, &st, &mx);
  bbuf o = {0};
  js_fmt(&c, &o, "{\"maxOp\":%lld,\"clock\":{", (long long)doc->max_op);
  /* clock: actorId -> last seq, in order of first appearance in the change columns */
  int first = 1;
  for (size_t i = 0; i < st.nchg; i++) {
    const int64_t a = st.chg[i].actor.v;
    int later = 0;
    for (size_t j = i + 1; j < st.nchg; j++) if (st.chg[j].actor.v == a) later = 1;
    if (later) continue;
    char ab[130];
    hex_actor(st.actors[a], st.actor_lens[a], ab);
    if (!first) bb_byte(&c, &o, ',');
    first = 0;
    js_fmt(&c, &o, "\"%s\":%lld", ab, (long long)st.chg[i].seq.v);
  }
  js_raw(&c, &o, "},\"deps\":[");
  for (size_t i = 0; i < st.nheads; i++) {
    if (i) bb_byte(&c, &o, ',');
    js_hex(&c, &o, st.heads + 32 * i, 32);
  }
  js_fmt(&c, &o, "],\"pendingChanges\":%zu,\"diffs\":", doc->nqueue);
  js_node(&c, &o, &st, root);
  bb_byte(&c, &o, '}');
  char *s = (char *)malloc(o.n + 1);
  memcpy(s, o.p, o.n);
  s[o.n] = 0;
  afree_all(&c);
  return s;
}

/* ---- flat export of a decoded document (host check of the engine's patch scan) ---- */
oc_export *oc_doc_export(const uint8_t *buf, size_t len, char *err, size_t errcap) {
  ctx_t *c = (ctx_t *)calloc(1, sizeof(ctx_t));
  if (setjmp(c->jb)) { set_err(c, err, errcap); afree_all(c); free(c); return NULL; }
  uint8_t *copy = (uint8_t *)amalloc(c, len + 1);
  memcpy(copy, buf, len);
  docst_t *st = (docst_t *)amalloc(c, sizeof(docst_t));
  decode_doc(c, copy, len, st);
  oc_export *e = (oc_export *)amalloc(c, sizeof(oc_export));
  memset(e, 0, sizeof *e);
  e->priv = c;
  e->nops = st->nops;
  e->ops = (oc_op *)amalloc(c, sizeof(oc_op) * (st->nops + 1));
  size_t ns = 0;
  for (size_t i = 0; i < st->nops; i++) ns += st->ops[i].nsucc;
  e->succ_ctr = (int64_t *)amalloc(c, sizeof(int64_t) * (ns + 1));
  e->succ_actor = (int32_t *)amalloc(c, sizeof(int32_t) * (ns + 1));
  size_t k = 0;
  for (size_t i = 0; i < st->nops; i++) {
    const op_t *op = &st->ops[i];
    oc_op *o = &e->ops[i];
    o->obj_ctr = op->obj_ctr.null ? -1 : op->obj_ctr.v;
    o->obj_actor = op->obj_actor.null ? -1 : (int32_t)op->obj_actor.v;
    o->key_ctr = op->key_ctr.null ? -1 : op->key_ctr.v;
    o->key_actor = op->key_actor.null ? -1 : (int32_t)op->key_actor.v;
    o->key = op->key_str.p;
    o->key_len = op->key_str.null ? -1 : (int32_t)op->key_str.n;
    o->id_ctr = op->id_ctr.v;
    o->id_actor = (int32_t)op->id_actor.v;
    o->insert = op->insert;
    o->action = op->action.null ? -1 : op->action.v;
    o->val_len = op->val_len.null ? 0 : op->val_len.v;
    o->val = op->val_raw;
    o->val_n = op->val_raw_n;
    o->nsucc = op->nsucc;
    o->succ_off = (uint32_t)k;
    for (uint32_t j = 0; j < op->nsucc; j++, k++) {
      e->succ_ctr[k] = op->succ_ctr[j].v;
      e->succ_actor[k] = (int32_t)op->succ_actor[j].v;
    }
  }
  e->nactors = st->nactors;
  e->actors = st->actors;
  e->actor_lens = st->actor_lens;
  e->nchg = st->nchg;
  e->chg_actor = (int64_t *)amalloc(c, sizeof(int64_t) * (st->nchg + 1));
  e->chg_seq = (int64_t *)amalloc(c, sizeof(int64_t) * (st->nchg + 1));
  for (size_t i = 0; i < st->nchg; i++) { e->chg_actor[i] = st->chg[i].actor.v; e->chg_seq[i] = st->chg[i].seq.v; }
  return e;
}

void oc_export_free(oc_export *e) {
  if (!e) return;
  ctx_t *c = (ctx_t *)e->priv;
  afree_all(c);
  free(c);
}
