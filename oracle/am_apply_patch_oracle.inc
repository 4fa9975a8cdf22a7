/* am_apply_patch_oracle.inc -- CPU restatement of the patch that Backend.applyChanges returns
 * (SURVEY.md §8 a20; included by am_oracle.c after am_patch_oracle.inc).
 *
 * TEST INFRASTRUCTURE ONLY. Restates, sequentially and literally, over the document as one op
 * block (the reference splits blocks at 600 ops; its block metadata only accelerates the seek):
 *   applyChanges (fn) / applyOps                       new.js:1550-1597, 1304-1380
 *   seekToOp / seekWithinBlock                         new.js:50-192, 227-317
 *   mergeDocChangeOps                                  new.js:1052-1290
 *   updatePatchProperty (incremental and whole-doc)    new.js:884-1040
 *   appendEdit / appendUpdate / convertInsertToUpdate  new.js:747-869
 *   setupPatches                                       new.js:1461-1528
 *   objectMeta as documentPatch leaves it at load      new.js:1604-1635, 1707, 1748
 * The seek keeps the reference's per-column decoder positions (e.g. the key seek of a non-root
 * object reads objActor/objCtr one op ahead of keyStr, new.js:78-90); mergeDocChangeOps then
 * walks forward exactly as the reference does. The replayed op sequence is checked against the
 * per-op merge of apply_changes.
 *
 * objectMeta: the objects (parent, parentKey, type) follow from the make ops of the document; the
 * children snapshots are per handle, as the reference carries them across calls (new.js:1812,
 * 1857): documentPatch's after load / init, then whatever the last updatePatchProperty of each
 * key left (oc_doc.pm, written back after every successful call). Pinned by the applyChanges
 * patches in tests/golden/docs.json and tests/golden/objmeta.json (produced by the reference).
 */

/* ---- objectMeta (new.js:894-931) ---- */
typedef struct {
  int64_t ctr, actor; /* opId of the value */
  int kind;           /* 1: value of a set op, 2: object {objectId, type} */
  const op_t *op;
  int64_t octr, oactor;
  const char *otype;
} mval;
typedef struct {
  int is_str; const uint8_t *key; uint32_t keyn; int64_t ec, ea; /* elemId */
  mval *v; size_t n, cap;
} mkey;
typedef struct mobj {
  int64_t ctr, actor; /* -1, -1: _root */
  int has_parent; int64_t pctr, pactor;
  int pk_str; const uint8_t *pkey; uint32_t pkeyn; int64_t pk_ec, pk_ea; /* parentKey */
  const char *type;
  mkey *ch; size_t nch, capch;
  struct mobj *next;
} mobj;
typedef struct { mobj *head; } mreg;

static mobj *meta_find(mreg *m, int64_t ctr, int64_t actor) {
  for (mobj *o = m->head; o; o = o->next) if (o->ctr == ctr && o->actor == actor) return o;
  return NULL;
}
static mobj *meta_new(ctx_t *c, mreg *m, int64_t ctr, int64_t actor, const char *type) {
  mobj *o = (mobj *)acalloc(c, sizeof(mobj));
  o->ctr = ctr; o->actor = actor; o->type = type;
  o->next = m->head;
  m->head = o;
  return o;
}
/* elemId of an op: its string key when truthy, else `${ctr}@${actor}` (new.js:888-890) */
typedef struct { int is_str; const uint8_t *key; uint32_t keyn; int64_t ec, ea; } elemid;
static elemid op_elemid(const op_t *op) {
  elemid e;
  e.is_str = !op->key_str.null && op->key_str.n > 0;
  e.key = op->key_str.p; e.keyn = op->key_str.n;
  e.ec = op->insert ? op->id_ctr.v : (op->key_ctr.null ? -1 : op->key_ctr.v);
  e.ea = op->insert ? op->id_actor.v : (op->key_actor.null ? -1 : op->key_actor.v);
  if (e.is_str) { e.ec = -1; e.ea = -1; }
  return e;
}
static int elemid_eq(elemid a, elemid b) {
  if (a.is_str != b.is_str) return 0;
  if (a.is_str) return a.keyn == b.keyn && (a.keyn == 0 || memcmp(a.key, b.key, a.keyn) == 0);
  return a.ec == b.ec && a.ea == b.ea;
}
static mkey *meta_child(ctx_t *c, mobj *o, elemid e, int create) {
  for (size_t i = 0; i < o->nch; i++) {
    elemid k = {o->ch[i].is_str, o->ch[i].key, o->ch[i].keyn, o->ch[i].ec, o->ch[i].ea};
    if (elemid_eq(k, e)) return &o->ch[i];
  }
  if (!create) return NULL;
  GROW(c, o->ch, o->nch, o->capch, mkey);
  mkey *k = &o->ch[o->nch++];
  memset(k, 0, sizeof *k);
  k->is_str = e.is_str; k->key = e.key; k->keyn = e.keyn; k->ec = e.ec; k->ea = e.ea;
  return k;
}
/* children[elemId][opId] = value, keeping the position of an existing opId (JS object keys) */
static void mkey_set(ctx_t *c, mkey *k, mval v) {
  for (size_t i = 0; i < k->n; i++)
    if (k->v[i].ctr == v.ctr && k->v[i].actor == v.actor) { k->v[i] = v; return; }
  GROW(c, k->v, k->n, k->cap, mval);
  k->v[k->n++] = v;
}

/* ---- propState (new.js:900-901, 941-965) ---- */
typedef struct {
  elemid e;
  const op_t **vis; size_t nvis, capvis; /* visibleOps */
  int has_child;
  int action; /* 0 none, 1 insert, 2 update, 3 remove */
  int has_cs; cstate *cs; size_t ncs, capcs; csucc *map; size_t nmap, capmap;
} pst;
typedef struct { pst *e; size_t n, cap; } pmap;
static pst *pmap_get(pmap *m, elemid e) {
  for (size_t i = 0; i < m->n; i++) if (elemid_eq(m->e[i].e, e)) return &m->e[i];
  return NULL;
}
static pst *pmap_add(ctx_t *c, pmap *m, elemid e) {
  GROW(c, m->e, m->n, m->cap, pst);
  pst *p = &m->e[m->n++];
  memset(p, 0, sizeof *p);
  p->e = e;
  return p;
}

/* ---- call state ---- */
struct apatch {
  docst_t st;    /* the replayed document */
  mreg meta;     /* objectMeta */
  preg patches;  /* patches: objectId -> object patch */
  int64_t *oid_ctr, *oid_actor; size_t noid, capoid; /* objectIds (Set, insertion order) */
};

static pnode *patch_for(ctx_t *c, apatch *ap, int64_t ctr, int64_t actor, const char *type) {
  pnode *p = reg_find(&ap->patches, ctr, actor);
  if (!p) {
    if (!type) unsupported(c, "patch for an object without objectMeta");
    p = reg_new(c, &ap->patches, ctr, actor, type);
  }
  return p;
}
static int is_list_type(const char *t) { return t && (strcmp(t, "list") == 0 || strcmp(t, "text") == 0); }
/* ops are copied when a patch or objectMeta keeps them (the replay mutates its doc op copies) */
static const op_t *op_keep(ctx_t *c, const op_t *op) {
  op_t *k = (op_t *)amalloc(c, sizeof(op_t));
  *k = *op;
  return k;
}

/* convertInsertToUpdate (new.js:838-869) */
static void convert_insert_to_update(ctx_t *c, pnode *p, int64_t index, elemid e) {
  pedit ups[64];
  size_t nu = 0;
  while (p->nedits > 0) {
    pedit *last = &p->edits[p->nedits - 1];
    if (last->action == ED_INSERT || last->action == ED_UPDATE) {
      if (last->index != index) fail(c, "last edit has unexpected index");
      if (nu == 64) unsupported(c, "too many updates of one list element");
      memmove(ups + 1, ups, sizeof(pedit) * nu);
      ups[0] = *last;
      nu++;
      p->nedits--;
      if (ups[0].action == ED_INSERT) break;
    } else {
      fail(c, "last edit has unexpected action");
    }
  }
  for (size_t i = 0; i < nu; i++) append_update(c, p, index, e.ec, e.ea, ups[i].op_ctr, ups[i].op_actor, ups[i].value, i == 0);
}

/* updatePatchProperty (new.js:884-1040). has_old = (oldSuccNum !== undefined). */
static void update_patch_property(ctx_t *c, apatch *ap, int64_t obj_ctr, int64_t obj_actor, const op_t *op_in, pmap *ps,
                                  int64_t list_index, int has_old, uint32_t old_succ, int whole_doc) {
  const op_t *op = op_keep(c, op_in);
  const int64_t action = op->action.v;
  if (action < 0 || action >= 8) unsupported(c, "unknown action %lld", (long long)action);
  const char *type = ACTION_OBJ_TYPE[action];
  const int64_t id_ctr = op->id_ctr.v, id_actor = op->id_actor.v;
  const elemid e = op_elemid(op);
  mobj *om = meta_find(&ap->meta, obj_ctr, obj_actor);
  if (!om) unsupported(c, "objectMeta[objectId] undefined");
  /* a new make* op: objectMeta[opId] and children[elemId][opId] (new.js:894-897) */
  if (action % 2 == 0 && !meta_find(&ap->meta, id_ctr, id_actor)) {
    mobj *nm = meta_new(c, &ap->meta, id_ctr, id_actor, type);
    nm->has_parent = 1; nm->pctr = obj_ctr; nm->pactor = obj_actor;
    nm->pk_str = e.is_str; nm->pkey = e.key; nm->pkeyn = e.keyn; nm->pk_ec = e.ec; nm->pk_ea = e.ea;
    mval v = {id_ctr, id_actor, 2, NULL, id_ctr, id_actor, type};
    mkey_set(c, meta_child(c, om, e, 1), v);
  }
  pst *s = pmap_get(ps, e);
  const int first_op = !s;
  if (!s) s = pmap_add(c, ps, e);
  const int overwritten = has_old && op->nsucc > 0;
  if (!overwritten) {
    GROW(c, s->vis, s->nvis, s->capvis, const op_t *);
    s->vis[s->nvis++] = op;
    s->has_child = s->has_child || (action % 2) == 0;
  }
  mkey *prev = meta_child(c, om, e, 0);
  if (s->has_child || (prev && prev->n > 0)) {
    mkey *k = meta_child(c, om, e, 1);
    k->n = 0; /* children[elemId] = values */
    for (size_t i = 0; i < s->nvis; i++) {
      const op_t *v = s->vis[i];
      const int64_t va = v->action.v;
      if (va == 1) {
        mval mv = {v->id_ctr.v, v->id_actor.v, 1, v, 0, 0, NULL};
        mkey_set(c, k, mv);
      } else if (va >= 0 && va < 8 && va % 2 == 0) {
        mval mv = {v->id_ctr.v, v->id_actor.v, 2, NULL, v->id_ctr.v, v->id_actor.v, ACTION_OBJ_TYPE[va]};
        mkey_set(c, k, mv);
      }
    }
  }
  /* patchKey / patchValue (new.js:933-977) */
  pval pv;
  memset(&pv, 0, sizeof pv);
  int64_t pk_ctr = 0, pk_actor = 0;
  const int64_t tag = op->val_len.null ? 0 : op->val_len.v;
  if (overwritten && action == 1 && (tag & 0x0f) == 8) {
    s->has_cs = 1;
    GROW(c, s->cs, s->ncs, s->capcs, cstate);
    cstate *cs = &s->cs[s->ncs++];
    cs->op_ctr = id_ctr; cs->op_actor = id_actor; cs->value = value_int(c, op); cs->nleft = 0;
    for (uint32_t k = 0; k < op->nsucc; k++) {
      size_t q = 0;
      while (q < s->nmap && !(s->map[q].succ_ctr == op->succ_ctr[k].v && s->map[q].succ_actor == op->succ_actor[k].v)) q++;
      if (q == s->nmap) { GROW(c, s->map, s->nmap, s->capmap, csucc); s->nmap++; }
      s->map[q].succ_ctr = op->succ_ctr[k].v; s->map[q].succ_actor = op->succ_actor[k].v; s->map[q].state = (int)(s->ncs - 1);
      int dup = 0;
      for (uint32_t j = 0; j < k; j++) if (op->succ_ctr[j].v == op->succ_ctr[k].v && op->succ_actor[j].v == op->succ_actor[k].v) dup = 1;
      if (!dup) cs->nleft++;
    }
  } else if (action == 5) {
    size_t q = 0;
    while (q < s->nmap && !(s->map[q].succ_ctr == id_ctr && s->map[q].succ_actor == id_actor)) q++;
    if (!s->has_cs || q == s->nmap) {
      char a[130];
      hex_actor(ap->st.actors[id_actor], ap->st.actor_lens[id_actor], a);
      fail(c, "increment operation %lld@%s for unknown counter", (long long)id_ctr, a);
    }
    cstate *cs = &s->cs[s->map[q].state];
    cs->value += inc_amount(c, op);
    cs->nleft--; /* delete counterState.succs[opId] (the map entry itself stays, new.js:959) */
    if (cs->nleft == 0) { pv.kind = PV_COUNTER; pv.counter = cs->value; pk_ctr = cs->op_ctr; pk_actor = cs->op_actor; }
  } else if (!overwritten) {
    if (action == 1) { pv.kind = PV_OP; pv.op = op; pk_ctr = id_ctr; pk_actor = id_actor; }
    else if (action % 2 == 0) {
      pv.kind = PV_CHILD; pv.child = patch_for(c, ap, id_ctr, id_actor, type);
      pk_ctr = id_ctr; pk_actor = id_actor;
    }
  }
  pnode *patch = patch_for(c, ap, obj_ctr, obj_actor, om->type);
  if (op->key_str.null) {
    /* list / text object (new.js:983-1033) */
    if (has_old && old_succ == 0 && !whole_doc && s->action == 1) {
      s->action = 2;
      convert_insert_to_update(c, patch, list_index, e);
    }
    if (pv.kind) {
      if (!s->action && (!has_old || whole_doc)) {
        s->action = 1;
        pedit ed;
        memset(&ed, 0, sizeof ed);
        ed.action = ED_INSERT; ed.index = list_index; ed.elem_ctr = e.ec; ed.elem_actor = e.ea;
        ed.op_ctr = pk_ctr; ed.op_actor = pk_actor; ed.value = pv;
        append_edit(c, patch, ed);
      } else if (s->action == 3) {
        pedit *last = patch->nedits ? &patch->edits[patch->nedits - 1] : NULL;
        if (!last || last->action != ED_REMOVE) fail(c, "last edit has unexpected type");
        if (last->count > 1) last->count--; else patch->nedits--;
        s->action = 2;
        append_update(c, patch, list_index, e.ec, e.ea, pk_ctr, pk_actor, pv, 1);
      } else {
        append_update(c, patch, list_index, e.ec, e.ea, pk_ctr, pk_actor, pv, !s->action);
        if (!s->action) s->action = 2;
      }
    } else if (has_old && old_succ == 0 && !s->action) {
      s->action = 3;
      pedit ed;
      memset(&ed, 0, sizeof ed);
      ed.action = ED_REMOVE; ed.index = list_index; ed.count = 1;
      append_edit(c, patch, ed);
    }
  } else if (pv.kind || !whole_doc) {
    /* map / table object (new.js:1035-1039) */
    pprop *pp = NULL;
    for (size_t k = 0; k < patch->nprops; k++)
      if (patch->props[k].keyn == op->key_str.n && (op->key_str.n == 0 || memcmp(patch->props[k].key, op->key_str.p, op->key_str.n) == 0))
        pp = &patch->props[k];
    if (!pp) {
      GROW(c, patch->props, patch->nprops, patch->capprops, pprop);
      pp = &patch->props[patch->nprops++];
      memset(pp, 0, sizeof *pp);
      pp->key = op->key_str.p; pp->keyn = op->key_str.n;
    } else if (first_op) {
      pp->n = 0;
    }
    if (pv.kind) {
      size_t k = 0;
      while (k < pp->n && !(pp->e[k].ctr == pk_ctr && pp->e[k].actor == pk_actor)) k++;
      if (k == pp->n) { GROW(c, pp->e, pp->n, pp->cap, pentry); pp->n++; }
      pp->e[k].ctr = pk_ctr; pp->e[k].actor = pk_actor; pp->e[k].v = pv;
    }
  }
}

/* objectMeta after documentPatch over the document (new.js:1604-1635, 1748) */
static void build_meta(ctx_t *c, apatch *ap) {
  const docst_t *st = &ap->st;
  meta_new(c, &ap->meta, -1, -1, "map");
  ap->patches.head = NULL;
  reg_new(c, &ap->patches, -1, -1, "map");
  pmap ps;
  memset(&ps, 0, sizeof ps);
  int64_t last_oa = -2, last_oc = -2;
  int elem_visible = 0;
  int64_t list_index = 0;
  for (size_t i = 0; i < st->nops; i++) {
    const op_t *op = &st->ops[i];
    const int64_t oa = op->obj_actor.null ? -1 : op->obj_actor.v, oc = op->obj_ctr.null ? -1 : op->obj_ctr.v;
    if (oa != last_oa || oc != last_oc) {
      last_oa = oa; last_oc = oc;
      memset(&ps, 0, sizeof ps);
      list_index = 0;
      elem_visible = 0;
    }
    if (op->insert && elem_visible) { elem_visible = 0; list_index++; }
    if (op->nsucc == 0) elem_visible = 1;
    update_patch_property(c, ap, oc, oa, op, &ps, list_index, 1, op->nsucc, 1);
  }
  ap->patches.head = NULL; /* the whole-document patch is not part of the result */
}

/* the children snapshots a previous call left (oc_doc.pm) replace documentPatch's */
static void meta_restore(ctx_t *c, apatch *ap, const oc_doc *doc) {
  for (mobj *o = ap->meta.head; o; o = o->next) o->nch = 0;
  for (size_t i = 0; i < doc->npm; i++) {
    const pm_key *pk = &doc->pm[i];
    mobj *om = meta_find(&ap->meta, pk->octr, pk->oactor);
    if (!om) unsupported(c, "persisted objectMeta names an unknown object");
    elemid e = {pk->is_str, pk->key, pk->keyn, pk->ec, pk->ea};
    mkey *k = meta_child(c, om, e, 1);
    k->n = 0;
    for (size_t j = 0; j < pk->n; j++) {
      const pm_val *pv = &pk->v[j];
      if (pv->kind == 2) {
        mobj *co = meta_find(&ap->meta, pv->ctr, pv->actor);
        if (!co) unsupported(c, "persisted objectMeta names an unknown child");
        mval mv = {pv->ctr, pv->actor, 2, NULL, pv->ctr, pv->actor, co->type};
        mkey_set(c, k, mv);
        continue;
      }
      const op_t *hit = NULL;
      for (size_t q = 0; q < ap->st.nops && !hit; q++) {
        const op_t *op = &ap->st.ops[q];
        const int64_t oa = op->obj_actor.null ? -1 : op->obj_actor.v, oc = op->obj_ctr.null ? -1 : op->obj_ctr.v;
        if (op->id_ctr.v == pv->ctr && op->id_actor.v == pv->actor && oa == pk->oactor && oc == pk->octr &&
            elemid_eq(op_elemid(op), e))
          hit = op;
      }
      if (!hit) unsupported(c, "persisted objectMeta names an unknown op");
      mval mv = {pv->ctr, pv->actor, 1, op_keep(c, hit), 0, 0, NULL};
      mkey_set(c, k, mv);
    }
  }
}

/* writes the call's children snapshots back to the handle (after the call succeeded) */
static void meta_save(apatch *ap, oc_doc *doc) {
  size_t n = 0;
  for (mobj *o = ap->meta.head; o; o = o->next) n += o->nch;
  pm_key *pm = (pm_key *)calloc(n + 1, sizeof(pm_key));
  size_t i = 0;
  for (mobj *o = ap->meta.head; o; o = o->next)
    for (size_t k = 0; k < o->nch; k++, i++) {
      const mkey *mk = &o->ch[k];
      pm[i].octr = o->ctr; pm[i].oactor = o->actor;
      pm[i].is_str = mk->is_str; pm[i].keyn = mk->keyn; pm[i].ec = mk->ec; pm[i].ea = mk->ea;
      pm[i].key = (uint8_t *)malloc(mk->keyn + 1);
      if (mk->keyn) memcpy(pm[i].key, mk->key, mk->keyn);
      pm[i].n = mk->n;
      pm[i].v = (pm_val *)malloc(sizeof(pm_val) * (mk->n + 1));
      for (size_t j = 0; j < mk->n; j++) { pm[i].v[j].ctr = mk->v[j].ctr; pm[i].v[j].actor = mk->v[j].actor; pm[i].v[j].kind = mk->v[j].kind; }
    }
  pm_free(doc->pm, doc->npm);
  doc->pm = pm;
  doc->npm = n;
  doc->meta_mode = 1;
}

/* ---- seekWithinBlock over one block (new.js:50-192), decoders as per-column cursors ---- */
typedef struct { int found; size_t skip; int64_t visible; } seekres;
typedef struct { const op_t *ops; size_t n, pos; } ccur;
static int cc_done(const ccur *d) { return d->pos >= d->n; }
static const op_t *cc_read(ccur *d) { return d->pos < d->n ? &d->ops[d->pos++] : NULL; }
static void cc_skip(ccur *d, size_t k) { d->pos = d->pos + k < d->n ? d->pos + k : d->n; }
/* JS `===` between nullable numbers */
static int nveq(nv a, nv b) { return a.null == b.null && (a.null || a.v == b.v); }
/* actor id string order a < b (undefined compares false) */
static int act_lt(const docst_t *st, int64_t a, int64_t b) {
  if (a < 0 || b < 0) return 0;
  return actor_cmp(st->actors[a], st->actor_lens[a], st->actors[b], st->actor_lens[b]) < 0;
}

typedef struct {
  nv obj_actor, obj_ctr, key_actor, key_ctr;
  ns key_str;
  int64_t id_actor, id_ctr;
  int insert;
} seekops;

static seekres seek_within_block(const docst_t *st, const op_t *ops, size_t n, const seekops *q) {
  ccur objA = {ops, n, 0}, objC = {ops, n, 0}, keyS = {ops, n, 0}, idA = {ops, n, 0}, idC = {ops, n, 0};
  ccur ins = {ops, n, 0}, act = {ops, n, 0}, succ = {ops, n, 0};
  seekres r = {1, 0, 0};
  int elem_visible = 0;
  nv next_obj_ctr = NUL;
  int64_t next_obj_actor = -1; /* actor index; -1 = null / undefined */
  nv next_id_ctr = NUL;
  int64_t next_id_actor = -1;
  int next_insert = 0;
  nv next_succ = NUL;
  const int64_t q_obj_actor = q->obj_actor.null ? -1 : q->obj_actor.v;
  if (!q->obj_ctr.null) {
    while (!cc_done(&objC) || !cc_done(&objA) || !cc_done(&act)) {
      const op_t *oc = cc_read(&objC), *oa = cc_read(&objA);
      next_obj_ctr = oc ? oc->obj_ctr : NUL;
      next_obj_actor = (oa && !oa->obj_actor.null) ? oa->obj_actor.v : -1;
      cc_skip(&act, 1);
      if (next_obj_ctr.null || next_obj_actor < 0 || next_obj_ctr.v < q->obj_ctr.v ||
          (next_obj_ctr.v == q->obj_ctr.v && act_lt(st, next_obj_actor, q_obj_actor))) {
        r.skip++;
      } else {
        break;
      }
    }
  }
  if (!nveq(next_obj_ctr, q->obj_ctr) || next_obj_actor != q_obj_actor) return r;
  if (!q->key_str.null) {
    cc_skip(&keyS, r.skip);
    while (!cc_done(&keyS)) {
      const op_t *oa = cc_read(&objA), *oc = cc_read(&objC), *ok = cc_read(&keyS);
      const int64_t noa = (oa && !oa->obj_actor.null) ? oa->obj_actor.v : -1;
      const nv noc = oc ? oc->obj_ctr : NUL;
      if (!ok->key_str.null && utf16_cmp(ok->key_str.p, ok->key_str.n, q->key_str.p, q->key_str.n) < 0 &&
          nveq(noc, q->obj_ctr) && noa == q_obj_actor) {
        r.skip++;
      } else {
        break;
      }
    }
    return r;
  }
  cc_skip(&idC, r.skip); cc_skip(&idA, r.skip); cc_skip(&ins, r.skip); cc_skip(&succ, r.skip);
#define READ_ID()                                                        \
  do {                                                                   \
    const op_t *a_ = cc_read(&idC), *b_ = cc_read(&idA);                 \
    next_id_ctr = a_ ? a_->id_ctr : NUL;                                 \
    next_id_actor = b_ ? b_->id_actor.v : -1;                            \
  } while (0)
#define READ_OBJ()                                                       \
  do {                                                                   \
    const op_t *a_ = cc_read(&objC), *b_ = cc_read(&objA);               \
    next_obj_ctr = a_ ? a_->obj_ctr : NUL;                               \
    next_obj_actor = (b_ && !b_->obj_actor.null) ? b_->obj_actor.v : -1; \
  } while (0)
#define READ_INS_SUCC()                                                  \
  do {                                                                   \
    const op_t *a_ = cc_read(&ins), *b_ = cc_read(&succ);                \
    next_insert = a_ ? a_->insert : 0;                                   \
    next_succ = b_ ? NV(b_->nsucc) : NUL;                                \
  } while (0)
#define VISIT()                                                          \
  do {                                                                   \
    if (next_insert) elem_visible = 0;                                   \
    if (!next_succ.null && next_succ.v == 0 && !elem_visible) {          \
      r.visible++;                                                       \
      elem_visible = 1;                                                  \
    }                                                                    \
  } while (0)
  READ_ID();
  READ_INS_SUCC();
  const int64_t q_key_actor = q->key_actor.null ? -1 : q->key_actor.v;
  if (q->insert) {
    if (!q->key_ctr.null && q->key_ctr.v > 0 && !q->key_actor.null) {
      r.skip++;
      while (!cc_done(&idC) && !cc_done(&idA) && (!nveq(next_id_ctr, q->key_ctr) || next_id_actor != q_key_actor)) {
        VISIT();
        READ_ID();
        READ_OBJ();
        READ_INS_SUCC();
        if (nveq(next_obj_ctr, q->obj_ctr) && next_obj_actor == q_obj_actor) r.skip++; else break;
      }
      if (!nveq(next_obj_ctr, q->obj_ctr) || next_obj_actor != q_obj_actor || !nveq(next_id_ctr, q->key_ctr) ||
          next_id_actor != q_key_actor || !next_insert) {
        r.found = 0;
        return r;
      }
      VISIT();
      if (cc_done(&idC) || cc_done(&idA)) return r;
      READ_ID();
      READ_OBJ();
      READ_INS_SUCC();
    }
    /* skip list elements with a greater id than the new one, and non-insertions (new.js:145-163) */
    for (;;) {
      const int greater = !next_id_ctr.null &&
                          (next_id_ctr.v > q->id_ctr || (next_id_ctr.v == q->id_ctr && act_lt(st, q->id_actor, next_id_actor)));
      if (!((!next_insert || greater) && nveq(next_obj_ctr, q->obj_ctr) && next_obj_actor == q_obj_actor)) break;
      r.skip++;
      VISIT();
      if (!cc_done(&idC) && !cc_done(&idA)) {
        READ_ID();
        READ_OBJ();
        READ_INS_SUCC();
      } else {
        break;
      }
    }
  } else if (!q->key_ctr.null && q->key_ctr.v > 0 && !q->key_actor.null) {
    /* update of an existing element: seek to just before it (new.js:165-190) */
    while ((!next_insert || !nveq(next_id_ctr, q->key_ctr) || next_id_actor != q_key_actor) &&
           nveq(next_obj_ctr, q->obj_ctr) && next_obj_actor == q_obj_actor) {
      r.skip++;
      VISIT();
      if (!cc_done(&idC) && !cc_done(&idA)) {
        READ_ID();
        READ_OBJ();
        READ_INS_SUCC();
      } else {
        break;
      }
    }
    if (!nveq(next_obj_ctr, q->obj_ctr) || next_obj_actor != q_obj_actor || !nveq(next_id_ctr, q->key_ctr) ||
        next_id_actor != q_key_actor || !next_insert) {
      r.found = 0;
    }
  }
#undef READ_ID
#undef READ_OBJ
#undef READ_INS_SUCC
#undef VISIT
  return r;
}

/* seekToOp with one block (new.js:227-317) */
static seekres seek_to_op(ctx_t *c, const docst_t *st, const seekops *q) {
  seekres r = seek_within_block(st, st->ops, st->nops, q);
  if (!q->key_str.null) { r.visible = 0; return r; }
  if (!r.found) {
    char ab[130] = "null";
    if (!q->key_actor.null) hex_actor(st->actors[q->key_actor.v], st->actor_lens[q->key_actor.v], ab);
    fail(c, "Reference element not found: %lld@%s", (long long)q->key_ctr.v, ab);
  }
  return r;
}

/* ---- mergeDocChangeOps (new.js:1052-1290) ---- */
typedef struct { op_t *ops; int64_t *author; size_t n, pos; } cstream;
typedef struct { op_t *v; size_t n, cap; } opvec;
static void opv_push(ctx_t *c, opvec *o, const op_t *op) {
  GROW(c, o->v, o->n, o->cap, op_t);
  o->v[o->n++] = *op;
}
static void objids_add(ctx_t *c, apatch *ap, int64_t ctr, int64_t actor) {
  for (size_t i = 0; i < ap->noid; i++) if (ap->oid_ctr[i] == ctr && ap->oid_actor[i] == actor) return;
  if (ap->noid == ap->capoid) {
    size_t nc = ap->capoid ? 2 * ap->capoid : 8;
    int64_t *a = (int64_t *)amalloc(c, sizeof(int64_t) * nc), *b = (int64_t *)amalloc(c, sizeof(int64_t) * nc);
    if (ap->noid) { memcpy(a, ap->oid_ctr, sizeof(int64_t) * ap->noid); memcpy(b, ap->oid_actor, sizeof(int64_t) * ap->noid); }
    ap->oid_ctr = a; ap->oid_actor = b; ap->capoid = nc;
  }
  ap->oid_ctr[ap->noid] = ctr; ap->oid_actor[ap->noid] = actor; ap->noid++;
}

static size_t merge_doc_change_ops(ctx_t *c, apatch *ap, size_t *dpos, opvec *out, cstream *cs, int64_t list_index) {
  docst_t *st = &ap->st;
  const op_t *first = &cs->ops[cs->pos];
  const int insert = first->insert;
  const nv f_obj_actor = first->obj_actor, f_obj_ctr = first->obj_ctr;
  const int64_t obj_actor = f_obj_actor.null ? -1 : f_obj_actor.v, obj_ctr = f_obj_actor.null ? -1 : f_obj_ctr.v;
  const int64_t id_actor_index = cs->author[cs->pos];
  int found_list_elem = 0, elem_visible = 0;
  pmap ps;
  memset(&ps, 0, sizeof ps);
  op_t doc_op;
  memset(&doc_op, 0, sizeof doc_op);
  int have_doc = 0;
  if (*dpos < st->nops) { doc_op = st->ops[(*dpos)++]; have_doc = 1; }
  size_t consumed = have_doc ? 1 : 0;
  uint32_t doc_old_succ = have_doc ? doc_op.nsucc : 0;
  const size_t cap = cs->n + 1;
  const op_t **cops = (const op_t **)amalloc(c, sizeof(op_t *) * cap);
  uint8_t **seen = (uint8_t **)amalloc(c, sizeof(uint8_t *) * cap);
  size_t nc = 0;
  const op_t *change_op = NULL;
  int have_lck = 0;
  ns last_change_key = {NULL, 0, 1};
  objids_add(c, ap, obj_ctr, obj_actor);
  for (;;) {
    if (nc == 0) {
      found_list_elem = 0;
      while (cs->pos < cs->n) {
        const op_t *next = &cs->ops[cs->pos];
        if (!(next->id_actor.v == id_actor_index && next->insert == insert && nveq(next->obj_actor, f_obj_actor) &&
              nveq(next->obj_ctr, f_obj_ctr)))
          break;
        const op_t *last = nc > 0 ? cops[nc - 1] : NULL;
        int is_overwrite = 0;
        for (uint32_t i = 0; i < next->nsucc; i++)
          for (size_t k = 0; k < nc; k++)
            if (next->succ_actor[i].v == cops[k]->id_actor.v && next->succ_ctr[i].v == cops[k]->id_ctr.v) is_overwrite = 1;
        int take = 0;
        if (next == first) take = 1;
        else if (insert && last && next->key_str.null && nveq(next->key_actor, last->id_actor) && nveq(next->key_ctr, last->id_ctr))
          take = 1;
        else if (!insert && last && !next->key_str.null && !last->key_str.null && ns_eq(next->key_str, last->key_str) &&
                 !is_overwrite)
          take = 1;
        else if (!insert && last && next->key_str.null && last->key_str.null && nveq(next->key_actor, last->key_actor) &&
                 nveq(next->key_ctr, last->key_ctr) && !is_overwrite)
          take = 1;
        else if (!insert && !last && next->key_str.null && have_doc && doc_op.insert && doc_op.key_str.null &&
                 nveq(doc_op.id_actor, next->key_actor) && nveq(doc_op.id_ctr, next->key_ctr))
          take = 1;
        else if (!insert && !last && !next->key_str.null && have_lck &&
                 utf16_cmp(last_change_key.p, last_change_key.n, next->key_str.p, next->key_str.n) < 0)
          take = 1;
        if (!take) break;
        have_lck = !next->key_str.null;
        last_change_key = next->key_str;
        cops[nc] = next;
        seen[nc] = (uint8_t *)acalloc(c, next->nsucc + 1);
        nc++;
        cs->pos++; /* readNextChangeOp */
      }
    }
    if (nc > 0) change_op = cops[0];
    const int in_obj = have_doc && nveq(doc_op.obj_actor, change_op->obj_actor) && nveq(doc_op.obj_ctr, change_op->obj_ctr);
    const int key_matches = have_doc && !doc_op.key_str.null && !change_op->key_str.null && ns_eq(doc_op.key_str, change_op->key_str);
    const int elem_matches = have_doc && doc_op.key_str.null && change_op->key_str.null &&
                             ((!doc_op.insert && nveq(doc_op.key_actor, change_op->key_actor) && nveq(doc_op.key_ctr, change_op->key_ctr)) ||
                              (doc_op.insert && nveq(doc_op.id_actor, change_op->key_actor) && nveq(doc_op.id_ctr, change_op->key_ctr)));
    if (nc == 0 && !(in_obj && (key_matches || elem_matches))) break;
    int take_doc = 0;
    size_t take_chg = 0;
    if (insert || !in_obj || (doc_op.key_str.null && !change_op->key_str.null) ||
        (!doc_op.key_str.null && !change_op->key_str.null &&
         utf16_cmp(change_op->key_str.p, change_op->key_str.n, doc_op.key_str.p, doc_op.key_str.n) < 0)) {
      take_chg = nc;
      if (!in_obj && !found_list_elem && change_op->key_str.null && !change_op->insert) {
        char ab[130] = "undefined";
        if (!change_op->key_actor.null) hex_actor(st->actors[change_op->key_actor.v], st->actor_lens[change_op->key_actor.v], ab);
        fail(c, "could not find list element with ID: %lld@%s", (long long)change_op->key_ctr.v, ab);
      }
    } else if (key_matches || elem_matches || found_list_elem) {
      for (size_t oi = 0; oi < nc; oi++) {
        const op_t *op = cops[oi];
        for (uint32_t i = 0; i < op->nsucc; i++) {
          if (op->succ_actor[i].v == doc_op.id_actor.v && op->succ_ctr[i].v == doc_op.id_ctr.v) {
            add_succ(c, st, &doc_op, op->id_ctr.v, id_actor_index);
            seen[oi][i] = 1;
            break;
          }
        }
      }
      if (elem_matches) found_list_elem = 1;
      if (found_list_elem && !elem_matches) {
        take_chg = nc;
      } else if (nc == 0 || doc_op.id_ctr.v < change_op->id_ctr.v ||
                 (doc_op.id_ctr.v == change_op->id_ctr.v && act_lt(st, doc_op.id_actor.v, id_actor_index))) {
        take_doc = 1;
        update_patch_property(c, ap, obj_ctr, obj_actor, &doc_op, &ps, list_index, 1, doc_old_succ, 0);
        /* a deletion whose preds have all been seen leaves no row (new.js:1205-1217) */
        for (size_t i = nc; i-- > 0;) {
          int deleted = 1;
          for (uint32_t j = 0; j < cops[i]->nsucc; j++) if (!seen[i][j]) deleted = 0;
          if (cops[i]->action.v == 3 && deleted) {
            memmove(cops + i, cops + i + 1, sizeof(op_t *) * (nc - i - 1));
            memmove(seen + i, seen + i + 1, sizeof(uint8_t *) * (nc - i - 1));
            nc--;
          }
        }
      } else if (doc_op.id_ctr.v == change_op->id_ctr.v && doc_op.id_actor.v == id_actor_index) {
        char ab[130];
        hex_actor(st->actors[id_actor_index], st->actor_lens[id_actor_index], ab);
        fail(c, "duplicate operation ID: %lld@%s", (long long)change_op->id_ctr.v, ab);
      } else {
        take_chg = 1;
      }
    } else {
      take_doc = 1;
    }
    if (take_doc) {
      opv_push(c, out, &doc_op);
      if (doc_op.insert && elem_visible) { elem_visible = 0; list_index++; }
      if (doc_op.nsucc == 0) elem_visible = 1;
      if (*dpos < st->nops) {
        doc_op = st->ops[(*dpos)++];
        consumed++;
        doc_old_succ = doc_op.nsucc;
      } else {
        have_doc = 0;
      }
    }
    if (take_chg > 0) {
      for (size_t i = 0; i < take_chg; i++) {
        const op_t *op = cops[i];
        for (uint32_t j = 0; j < op->nsucc; j++)
          if (!seen[i][j]) {
            char ab[130];
            hex_actor(st->actors[op->succ_actor[j].v], st->actor_lens[op->succ_actor[j].v], ab);
            fail(c, "no matching operation for pred: %lld@%s", (long long)op->succ_ctr[j].v, ab);
          }
        /* appendOperation writes the change op into the document columns: pred columns have other
         * ids than succ, so the row has no succ */
        op_t row = *op;
        row.nsucc = 0;
        row.succ_actor = row.succ_ctr = NULL;
        opv_push(c, out, &row);
        update_patch_property(c, ap, obj_ctr, obj_actor, &row, &ps, list_index, 0, 0, 0);
        if (op->insert) { elem_visible = 0; list_index++; }
        else elem_visible = 1;
      }
      memmove(cops, cops + take_chg, sizeof(op_t *) * (nc - take_chg));
      memmove(seen, seen + take_chg, sizeof(uint8_t *) * (nc - take_chg));
      nc -= take_chg;
    }
  }
  if (have_doc) opv_push(c, out, &doc_op);
  return consumed;
}

/* applyOps (new.js:1304-1380) */
static void apply_ops_patch(ctx_t *c, apatch *ap, cstream *cs) {
  docst_t *st = &ap->st;
  const op_t *first = &cs->ops[cs->pos];
  seekops q;
  q.obj_actor = first->obj_actor; q.obj_ctr = first->obj_ctr;
  q.key_actor = first->key_actor; q.key_ctr = first->key_ctr;
  q.key_str = first->key_str;
  q.id_actor = first->id_actor.v; q.id_ctr = first->id_ctr.v;
  q.insert = first->insert;
  const seekres r = seek_to_op(c, st, &q);
  opvec out = {NULL, 0, 0};
  for (size_t i = 0; i < r.skip; i++) opv_push(c, &out, &st->ops[i]);
  size_t dpos = r.skip;
  const size_t consumed = merge_doc_change_ops(c, ap, &dpos, &out, cs, r.visible);
  for (size_t i = r.skip + consumed; i < st->nops; i++) opv_push(c, &out, &st->ops[i]);
  st->ops = out.v;
  st->nops = out.n;
  st->capops = out.cap;
}

/* One applyChanges() pass over its applied changes (new.js:1588-1591); apply_changes calls this
 * before running the same pass on the main state. */
static void ap_pass(ctx_t *c, apatch *ap, change_t **applied, size_t na) {
  docst_t *st = &ap->st;
  size_t total = 0;
  op_t **per = (op_t **)amalloc(c, sizeof(op_t *) * (na + 1));
  size_t *pern = (size_t *)amalloc(c, sizeof(size_t) * (na + 1));
  int64_t *auth = (int64_t *)amalloc(c, sizeof(int64_t) * (na + 1));
  for (size_t ai = 0; ai < na; ai++) {
    change_t *ch = applied[ai];
    int64_t self = actor_index(st, ch->actor, ch->actor_len);
    if (self < 0) {
      const uint8_t **na_ = (const uint8_t **)amalloc(c, sizeof(uint8_t *) * (st->nactors + 1));
      uint32_t *nl_ = (uint32_t *)amalloc(c, sizeof(uint32_t) * (st->nactors + 1));
      memcpy(na_, st->actors, sizeof(uint8_t *) * st->nactors);
      memcpy(nl_, st->actor_lens, sizeof(uint32_t) * st->nactors);
      na_[st->nactors] = ch->actor;
      nl_[st->nactors] = ch->actor_len;
      st->actors = na_;
      st->actor_lens = nl_;
      self = (int64_t)st->nactors++;
    }
    int64_t *table = (int64_t *)amalloc(c, sizeof(int64_t) * ch->nactors);
    for (size_t t = 0; t < ch->nactors; t++) {
      table[t] = actor_index(st, ch->actors[t], ch->actor_lens[t]);
      if (table[t] < 0) unsupported(c, "actor not known (replay)");
    }
    colbuf cb[16];
    decode_columns_generic(c, ch->cols, ch->ncols, CHANGE_COLS, 16, cb);
    read_ops(c, cb, 0, &per[ai], &pern[ai]);
    for (size_t oi = 0; oi < pern[ai]; oi++) {
      op_t *o = &per[ai][oi];
      nv *acts[3] = {&o->obj_actor, &o->key_actor, &o->chld_actor};
      for (int k = 0; k < 3; k++) if (!acts[k]->null) acts[k]->v = table[acts[k]->v];
      for (uint32_t p = 0; p < o->nsucc; p++) if (!o->succ_actor[p].null) o->succ_actor[p].v = table[o->succ_actor[p].v];
      o->id_actor = NV(self);
      o->id_ctr = NV(ch->start_op + (int64_t)oi);
    }
    auth[ai] = self;
    total += pern[ai];
  }
  cstream cs;
  cs.ops = (op_t *)amalloc(c, sizeof(op_t) * (total + 1));
  cs.author = (int64_t *)amalloc(c, sizeof(int64_t) * (total + 1));
  cs.n = 0;
  cs.pos = 0;
  for (size_t ai = 0; ai < na; ai++)
    for (size_t oi = 0; oi < pern[ai]; oi++) { cs.ops[cs.n] = per[ai][oi]; cs.author[cs.n] = auth[ai]; cs.n++; }
  while (cs.pos < cs.n) apply_ops_patch(c, ap, &cs);
}

/* setupPatches (new.js:1461-1528) */
static void setup_patches(ctx_t *c, apatch *ap) {
  for (size_t oi = 0; oi < ap->noid; oi++) {
    int64_t octr = ap->oid_ctr[oi], oact = ap->oid_actor[oi];
    mobj *meta = meta_find(&ap->meta, octr, oact), *child = NULL;
    if (!meta) unsupported(c, "objectMeta missing in setupPatches");
    int exists = 0;
    for (;;) {
      mkey *kids = NULL;
      int has_children = 0;
      if (child) {
        elemid pk = {child->pk_str, child->pkey, child->pkeyn, child->pk_ec, child->pk_ea};
        kids = meta_child(c, meta, pk, 0);
        if (!kids) unsupported(c, "children of parentKey undefined");
        has_children = kids->n > 0;
      }
      pnode *patch = patch_for(c, ap, octr, oact, meta->type);
      if (child && has_children) {
        if (is_list_type(meta->type)) {
          for (size_t k = 0; k < patch->nedits; k++) {
            const pedit *ed = &patch->edits[k];
            if (ed->action != ED_INSERT && ed->action != ED_UPDATE) continue; /* edit.opId */
            for (size_t j = 0; j < kids->n; j++)
              if (kids->v[j].ctr == ed->op_ctr && kids->v[j].actor == ed->op_actor) exists = 1;
          }
          if (!exists) {
            seekops q;
            q.obj_actor = NV(oact); q.obj_ctr = NV(octr);
            q.key_actor = NV(child->pk_ea); q.key_ctr = NV(child->pk_ec);
            q.key_str.p = NULL; q.key_str.n = 0; q.key_str.null = 1;
            q.id_actor = -1; q.id_ctr = 0;
            q.insert = 0;
            const seekres r = seek_to_op(c, &ap->st, &q);
            for (size_t j = 0; j < kids->n; j++) {
              const mval *mv = &kids->v[j];
              pedit ed;
              memset(&ed, 0, sizeof ed);
              if (mv->kind == 2) { ed.value.kind = PV_CHILD; ed.value.child = patch_for(c, ap, mv->octr, mv->oactor, mv->otype); }
              else { ed.value.kind = PV_OP; ed.value.op = mv->op; }
              ed.action = ED_UPDATE; ed.index = r.visible; ed.op_ctr = mv->ctr; ed.op_actor = mv->actor;
              append_edit(c, patch, ed);
            }
          }
        } else {
          pprop *pp = NULL;
          for (size_t k = 0; k < patch->nprops; k++)
            if (patch->props[k].keyn == child->pkeyn && (child->pkeyn == 0 || memcmp(patch->props[k].key, child->pkey, child->pkeyn) == 0))
              pp = &patch->props[k];
          if (!pp) {
            GROW(c, patch->props, patch->nprops, patch->capprops, pprop);
            pp = &patch->props[patch->nprops++];
            memset(pp, 0, sizeof *pp);
            pp->key = child->pkey; pp->keyn = child->pkeyn;
          }
          for (size_t j = 0; j < kids->n; j++) {
            const mval *mv = &kids->v[j];
            size_t k = 0;
            while (k < pp->n && !(pp->e[k].ctr == mv->ctr && pp->e[k].actor == mv->actor)) k++;
            if (k < pp->n) { exists = 1; continue; }
            GROW(c, pp->e, pp->n, pp->cap, pentry);
            pentry *pe = &pp->e[pp->n++];
            pe->ctr = mv->ctr; pe->actor = mv->actor;
            memset(&pe->v, 0, sizeof pe->v);
            if (mv->kind == 2) { pe->v.kind = PV_CHILD; pe->v.child = patch_for(c, ap, mv->octr, mv->oactor, mv->otype); }
            else { pe->v.kind = PV_OP; pe->v.op = mv->op; }
          }
        }
      }
      if (exists || !meta->has_parent || (child && !has_children)) break;
      child = meta;
      octr = meta->pctr; oact = meta->pactor;
      meta = meta_find(&ap->meta, octr, oact);
      if (!meta) unsupported(c, "objectMeta of parent missing");
    }
  }
}

/* Backend.applyChanges(doc, changes) -> the returned patch as JSON (malloc'd); the document is
 * updated as by oc_doc_apply. Returns NULL on error. */
char *oc_doc_apply_patch(oc_doc *doc, const uint8_t *const *bufs, const size_t *lens, size_t n, char *err, size_t errcap) {
  CTX_BEGIN(c) { g_ap = NULL; set_err(&c, err, errcap); afree_all(&c); return NULL; }
  docst_t st;
  /* decode from a private copy: apply_changes replaces (frees) doc->state, and the patch keeps
   * pointers into the decoded bytes (actor ids, keys, values) */
  if (doc->state) {
    uint8_t *copy = (uint8_t *)amalloc(&c, doc->state_n + 1);
    memcpy(copy, doc->state, doc->state_n);
    decode_doc(&c, copy, doc->state_n, &st);
  } else {
    empty_state(&st);
  }
  apatch *ap = (apatch *)acalloc(&c, sizeof(apatch));
  ap->st = st;
  ap->st.ops = (op_t *)amalloc(&c, sizeof(op_t) * (st.nops + 1));
  if (st.nops) memcpy(ap->st.ops, st.ops, sizeof(op_t) * st.nops);
  ap->st.capops = st.nops;
  if (doc->meta_mode == 2) unsupported(&c, "objectMeta after a patchless applyChanges is not tracked by the oracle");
  build_meta(&c, ap);
  if (doc->meta_mode == 1) meta_restore(&c, ap, doc);
  reg_new(&c, &ap->patches, -1, -1, "map"); /* patches = {_root: ...} */
  g_ap = ap;
  apply_changes(&c, doc, &st, bufs, lens, n);
  g_ap = NULL;
  /* the replay must have produced the op sequence of the per-op merge */
  if (ap->st.nops != st.nops) unsupported(&c, "replay diverged (%zu vs %zu ops)", ap->st.nops, st.nops);
  for (size_t i = 0; i < st.nops; i++) {
    const op_t *a = &ap->st.ops[i], *b = &st.ops[i];
    int same = a->id_ctr.v == b->id_ctr.v && a->id_actor.v == b->id_actor.v && a->nsucc == b->nsucc;
    for (uint32_t k = 0; same && k < a->nsucc; k++)
      same = a->succ_ctr[k].v == b->succ_ctr[k].v && a->succ_actor[k].v == b->succ_actor[k].v;
    if (!same) unsupported(&c, "replay diverged at op %zu", i);
  }
  setup_patches(&c, ap);
  meta_save(ap, doc);
  bbuf o = {0};
  js_fmt(&c, &o, "{\"maxOp\":%lld,\"clock\":{", (long long)doc->max_op);
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
  js_node(&c, &o, &ap->st, reg_find(&ap->patches, -1, -1));
  bb_byte(&c, &o, '}');
  char *s = (char *)malloc(o.n + 1);
  memcpy(s, o.p, o.n);
  s[o.n] = 0;
  afree_all(&c);
  return s;
}
