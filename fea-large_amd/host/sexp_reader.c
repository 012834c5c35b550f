/*
 * sexp_reader.c -- streaming reader / writer for the task deck grammar.
 *
 * The reference parses the deck into an AST with libsexp and walks it
 * (solver-large/sexp_loader.c:249-327).  libsexp is not part of the
 * reference tree, and the 10M-element decks this build targets are GB-sized
 * as text, so this reader consumes the token stream directly and fills flat
 * arrays; nothing is kept but the current list's attributes.
 *
 * Grammar (from the five decks under solver-large/data and the emitter
 * utilities/tetgenProcessor/FEATask.hs:177-207):
 *   ';' starts a comment to end of line; lists are ( head item* );
 *   ':key value' pairs are attributes of the enclosing list; symbols are
 *   compared without regard to case (`yes` vs "YES", sexp_loader.c:90);
 *   numbers go through strtod, so coordinates round exactly as written.
 */
#include <ctype.h>
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fea_host.h"

#define TOK_MAX 256
#define ATTR_MAX 16

typedef struct {
  FILE *f;
  int line;
  char err[256];
  int n_element_material;        /* ids read by (element-materials ...), -1: no such section */
} reader;

enum { T_EOF, T_OPEN, T_CLOSE, T_ATOM };

static int next_token(reader *r, char *buf)
{
  int c;
  for (;;) {
    c = fgetc(r->f);
    if (c == EOF) return T_EOF;
    if (c == '\n') { r->line++; continue; }
    if (isspace(c)) continue;
    if (c == ';') {
      while ((c = fgetc(r->f)) != EOF && c != '\n') {}
      if (c == '\n') r->line++;
      continue;
    }
    break;
  }
  if (c == '(') return T_OPEN;
  if (c == ')') return T_CLOSE;
  {
    int n = 0;
    if (c == '"') {
      while ((c = fgetc(r->f)) != EOF && c != '"')
        if (n < TOK_MAX - 1) buf[n++] = (char)c;
    } else {
      do {
        if (n < TOK_MAX - 1) buf[n++] = (char)c;
        c = fgetc(r->f);
      } while (c != EOF && !isspace(c) && c != '(' && c != ')' && c != ';');
      if (c != EOF) ungetc(c, r->f);
    }
    buf[n] = 0;
  }
  return T_ATOM;
}

static int ieq(const char *a, const char *b)
{
  for (; *a && *b; ++a, ++b)
    if (toupper((unsigned char)*a) != toupper((unsigned char)*b)) return 0;
  return *a == 0 && *b == 0;
}

typedef struct { char key[48]; char val[TOK_MAX]; } attr;

static const char *attr_get(const attr *a, int n, const char *key)
{
  int i;
  for (i = 0; i < n; ++i)
    if (ieq(a[i].key, key)) return a[i].val;
  return NULL;
}

static int fail(reader *r, const char *msg)
{
  snprintf(r->err, sizeof(r->err), "line %d: %s", r->line, msg);
  return -1;
}

static int need_num(reader *r, const attr *a, int n, const char *key, double *out)
{
  const char *v = attr_get(a, n, key);
  char *end;
  if (!v) { char m[96]; snprintf(m, sizeof m, "missing attribute :%s", key); return fail(r, m); }
  *out = strtod(v, &end);
  if (end == v) { char m[96]; snprintf(m, sizeof m, "attribute :%s is not a number", key); return fail(r, m); }
  return 0;
}

/* skips a list whose '(' has been consumed */
static int skip_list(reader *r)
{
  char buf[TOK_MAX];
  int depth = 1, t;
  while (depth > 0) {
    t = next_token(r, buf);
    if (t == T_EOF) return fail(r, "unexpected end of file");
    if (t == T_OPEN) depth++;
    else if (t == T_CLOSE) depth--;
  }
  return 0;
}

/* (nodes (x y z) ...)  sexp_loader.c:169-189 */
static int read_nodes(reader *r, fea_deck *d)
{
  char buf[TOK_MAX];
  size_t cap = 1024, n = 0;
  double *p = (double *)malloc(cap * 3 * sizeof(double));
  for (;;) {
    int t = next_token(r, buf), k;
    if (t == T_CLOSE) break;
    if (t != T_OPEN) { free(p); return fail(r, "node entry must be a list of three numbers"); }
    if (n == cap) { cap *= 2; p = (double *)realloc(p, cap * 3 * sizeof(double)); }
    for (k = 0; k < 3; ++k) {
      char *end;
      if (next_token(r, buf) != T_ATOM) { free(p); return fail(r, "node needs three coordinates"); }
      p[n * 3 + k] = strtod(buf, &end);
      if (end == buf) { free(p); return fail(r, "bad node coordinate"); }
    }
    if (next_token(r, buf) != T_CLOSE) { free(p); return fail(r, "node needs exactly three coordinates"); }
    n++;
  }
  free(d->nodes);
  d->nodes = p; d->nodes_count = (int)n;
  return 0;
}

/* (elements (n0 ... n_{npe-1}) ...)  sexp_loader.c:191-211; the element
 * type must already be known, as in the reference (:203-206)                */
static int read_elements(reader *r, fea_deck *d)
{
  char buf[TOK_MAX];
  int npe = d->nodes_per_element;
  size_t cap = 1024, n = 0;
  int *p = (int *)malloc(cap * npe * sizeof(int));
  for (;;) {
    int t = next_token(r, buf), k;
    if (t == T_CLOSE) break;
    if (t != T_OPEN) { free(p); return fail(r, "element entry must be a list of node ids"); }
    if (n == cap) { cap *= 2; p = (int *)realloc(p, cap * npe * sizeof(int)); }
    for (k = 0; k < npe; ++k) {
      char *end;
      if (next_token(r, buf) != T_ATOM) { free(p); return fail(r, "element has too few node ids"); }
      p[n * npe + k] = (int)strtol(buf, &end, 10);
      if (end == buf) { free(p); return fail(r, "bad node id in element"); }
    }
    if (next_token(r, buf) != T_CLOSE) { free(p); return fail(r, "element has too many node ids"); }
    n++;
  }
  free(d->elements);
  d->elements = p; d->elements_count = (int)n;
  return 0;
}

/* reads the attributes of a list whose head has been consumed, up to ')';
 * nested lists are handed to `nested` (may be NULL = skip)                  */
typedef int (*nested_fn)(reader *r, fea_deck *d);
static int read_list(reader *r, fea_deck *d);

static int read_attrs(reader *r, fea_deck *d, attr *a, int *na, int recurse)
{
  char buf[TOK_MAX];
  *na = 0;
  for (;;) {
    int t = next_token(r, buf);
    if (t == T_EOF) return fail(r, "unexpected end of file");
    if (t == T_CLOSE) return 0;
    if (t == T_OPEN) {
      if (recurse) { if (read_list(r, d)) return -1; }
      else if (skip_list(r)) return -1;
      continue;
    }
    if (buf[0] == ':') {
      char key[48];
      snprintf(key, sizeof key, "%s", buf + 1);
      t = next_token(r, buf);
      if (t == T_OPEN && ieq(key, "base")) {                 /* :base (bx by bz) of (transient ...): its atoms, blank-separated */
        size_t len = 0;
        buf[0] = 0;
        for (;;) {
          char tok[TOK_MAX];
          t = next_token(r, tok);
          if (t == T_CLOSE) break;
          if (t != T_ATOM || len + strlen(tok) + 2 > sizeof buf) return fail(r, ":base takes a list of three numbers");
          len += (size_t)snprintf(buf + len, sizeof buf - len, len ? " %s" : "%s", tok);
        }
        t = T_ATOM;
      }
      if (t == T_OPEN) { if (skip_list(r)) return -1; continue; }
      if (t != T_ATOM) return fail(r, "attribute without a value");
      if (*na < ATTR_MAX) {
        snprintf(a[*na].key, sizeof a[*na].key, "%s", key);
        snprintf(a[*na].val, sizeof a[*na].val, "%s", buf);
        (*na)++;
      }
    }
  }
}

/* (prescribed-displacements (presc-node :x :y :z :type :node-id) ...)
 * sexp_loader.c:213-246 */
static int read_prescribed(reader *r, fea_deck *d)
{
  char buf[TOK_MAX];
  size_t cap = 256, n = 0;
  int *node = (int *)malloc(cap * sizeof(int)), *type = (int *)malloc(cap * sizeof(int));
  double *val = (double *)malloc(cap * 3 * sizeof(double));
  int rc = 0;
  for (;;) {
    attr a[ATTR_MAX];
    int na, t = next_token(r, buf);
    double v;
    if (t == T_CLOSE) break;
    if (t != T_OPEN || next_token(r, buf) != T_ATOM || !ieq(buf, "presc-node")) {
      rc = fail(r, "expected (presc-node ...)"); break;
    }
    if ((rc = read_attrs(r, d, a, &na, 0))) break;
    if (n == cap) {
      cap *= 2;
      node = (int *)realloc(node, cap * sizeof(int));
      type = (int *)realloc(type, cap * sizeof(int));
      val = (double *)realloc(val, cap * 3 * sizeof(double));
    }
    if ((rc = need_num(r, a, na, "node-id", &v))) break; node[n] = (int)v;
    if ((rc = need_num(r, a, na, "x", &val[n * 3 + 0]))) break;
    if ((rc = need_num(r, a, na, "y", &val[n * 3 + 1]))) break;
    if ((rc = need_num(r, a, na, "z", &val[n * 3 + 2]))) break;
    if ((rc = need_num(r, a, na, "type", &v))) break; type[n] = (int)v;
    n++;
  }
  if (rc) { free(node); free(type); free(val); return rc; }
  free(d->presc_node); free(d->presc_type); free(d->presc_values);
  d->presc_node = node; d->presc_type = type; d->presc_values = val;
  d->prescribed_nodes_count = (int)n;
  return 0;
}

/* (surface-loads (pressure :value p :nodes (n ...)) (traction :x :y :z :nodes (n ...)) ...): no counterpart in the
 * reference, whose loader skips lists it does not know (sexp_loader.c:249-272).  Every face has the node count of
 * the first one; whether the nodes form a boundary face is checked by feahip_set_surface_loads. */
static int read_surface(reader *r, fea_deck *d)
{
  char buf[TOK_MAX];
  size_t cap = 64, n = 0;
  int npf = 0, rc = 0;
  int *nodes = (int *)malloc(cap * 8 * sizeof(int)), *kind = (int *)malloc(cap * sizeof(int));
  double *val = (double *)malloc(cap * 3 * sizeof(double));
  for (;;) {
    int t = next_token(r, buf), k = 0, got_nodes = 0, ids[8];
    double v[3] = {0, 0, 0};
    int have[3] = {0, 0, 0};
    if (t == T_CLOSE) break;
    if (t != T_OPEN || next_token(r, buf) != T_ATOM || !(ieq(buf, "pressure") || ieq(buf, "traction"))) {
      rc = fail(r, "expected (pressure ...) or (traction ...)"); break;
    }
    if (n == cap) {
      cap *= 2;
      nodes = (int *)realloc(nodes, cap * 8 * sizeof(int));
      kind = (int *)realloc(kind, cap * sizeof(int));
      val = (double *)realloc(val, cap * 3 * sizeof(double));
    }
    kind[n] = ieq(buf, "pressure") ? FEAHIP_LOAD_PRESSURE : FEAHIP_LOAD_TRACTION;
    for (;;) {
      char key[48], *end;
      t = next_token(r, buf);
      if (t == T_CLOSE) break;
      if (t != T_ATOM || buf[0] != ':') { rc = fail(r, "surface load: expected :key value"); break; }
      snprintf(key, sizeof key, "%s", buf + 1);
      if (ieq(key, "nodes")) {
        if (next_token(r, buf) != T_OPEN) { rc = fail(r, ":nodes must be a list of node ids"); break; }
        for (k = 0; (t = next_token(r, buf)) == T_ATOM; ++k) {
          if (k == 6) { rc = fail(r, "a face has at most 6 nodes"); break; }
          ids[k] = (int)strtol(buf, &end, 10);
          if (end == buf) { rc = fail(r, "bad node id in :nodes"); break; }
        }
        if (rc) break;
        if (t != T_CLOSE) { rc = fail(r, ":nodes must be a list of node ids"); break; }
        got_nodes = 1;
        continue;
      }
      if (next_token(r, buf) != T_ATOM) { rc = fail(r, "attribute without a value"); break; }
      {
        const int slot = ieq(key, "value") || ieq(key, "x") ? 0 : ieq(key, "y") ? 1 : ieq(key, "z") ? 2 : -1;
        if (slot < 0) continue;
        v[slot] = strtod(buf, &end);
        if (end == buf) { rc = fail(r, "surface load value is not a number"); break; }
        have[slot] = 1;
      }
    }
    if (rc) break;
    if (!got_nodes || k == 0) { rc = fail(r, "surface load without :nodes"); break; }
    if (n == 0) npf = k;
    else if (k != npf) { rc = fail(r, "every loaded face must have the same number of nodes"); break; }
    if (kind[n] == FEAHIP_LOAD_PRESSURE ? !have[0] : !(have[0] && have[1] && have[2])) {
      rc = fail(r, kind[n] == FEAHIP_LOAD_PRESSURE ? "pressure needs :value" : "traction needs :x :y :z"); break;
    }
    if (kind[n] == FEAHIP_LOAD_PRESSURE) v[1] = v[2] = 0;
    memcpy(nodes + n * 8, ids, sizeof(int) * (size_t)k);
    memcpy(val + n * 3, v, sizeof v);
    n++;
  }
  if (rc) { free(nodes); free(kind); free(val); return rc; }
  {
    size_t i;
    for (i = 0; i < n; ++i) memmove(nodes + i * (size_t)npf, nodes + i * 8, sizeof(int) * (size_t)npf);   /* pack */
  }
  free(d->surface_nodes); free(d->surface_kind); free(d->surface_values);
  d->surface_nodes = nodes; d->surface_kind = kind; d->surface_values = val;
  d->surface_faces_count = (int)n; d->surface_nodes_per_face = npf;
  return 0;
}

/* (x y z) whose '(' has not been consumed */
static int read_vec3(reader *r, double *v, const char *what)
{
  char buf[TOK_MAX], m[96], *end;
  int k;
  snprintf(m, sizeof m, "contact: %s must be a list of three numbers", what);
  if (next_token(r, buf) != T_OPEN) return fail(r, m);
  for (k = 0; k < 3; ++k) {
    if (next_token(r, buf) != T_ATOM) return fail(r, m);
    v[k] = strtod(buf, &end);
    if (end == buf || *end) return fail(r, m);
  }
  if (next_token(r, buf) != T_CLOSE) return fail(r, m);
  return 0;
}

/* (contact :penalty e :augment k :gap-tolerance g (faces (n ...) ...) (plane :point (..) :normal (..) :travel (..))
 * (sphere :center (..) :radius r :travel (..) :inside t) (cylinder :point (..) :axis (..) :radius r :travel (..) :inside t)
 * ...) inside (boundary-conditions ...): the faces and obstacles of feahip_set_contact, obstacles in deck order.  No
 * counterpart in the reference.  Whether the nodes form boundary faces is checked by feahip_set_contact; what can be
 * told from the text alone is refused here. */
static int read_contact(reader *r, fea_deck *d)
{
  char buf[TOK_MAX], key[48], *end;
  int nobs = 0, npf = 0, nfaces = 0, rc = 0, have_penalty = 0, have_faces = 0, t;
  size_t cap = 64;
  int *nodes = (int *)malloc(cap * 8 * sizeof(int));
  int *kind = (int *)malloc(FEAHIP_MAX_OBSTACLES * sizeof(int));
  double *geom = (double *)calloc(FEAHIP_MAX_OBSTACLES * 10, sizeof(double));
  double penalty = 0, gap = 0, augment = 0;
  if (!nodes || !kind || !geom) { free(nodes); free(kind); free(geom); return fail(r, "out of memory reading (contact ...)"); }
  while (!rc) {
    t = next_token(r, buf);
    if (t == T_CLOSE) break;
    if (t == T_EOF) { rc = fail(r, "unexpected end of file"); break; }
    if (t == T_ATOM) {                                         /* :penalty :augment :gap-tolerance */
      double v;
      if (buf[0] != ':') { rc = fail(r, "contact: expected :key value or a list"); break; }
      snprintf(key, sizeof key, "%s", buf + 1);
      if (next_token(r, buf) != T_ATOM) { rc = fail(r, "attribute without a value"); break; }
      v = strtod(buf, &end);
      if (end == buf || *end) { rc = fail(r, "contact: attribute is not a number"); break; }
      if (ieq(key, "penalty")) { penalty = v; have_penalty = 1; }
      else if (ieq(key, "augment")) augment = v;
      else if (ieq(key, "gap-tolerance")) gap = v;
      else { rc = fail(r, "contact: unknown attribute (:penalty :augment :gap-tolerance)"); break; }
      continue;
    }
    if (next_token(r, buf) != T_ATOM) { rc = fail(r, "contact: expected (faces ...), (plane ...), (sphere ...) or (cylinder ...)"); break; }
    if (ieq(buf, "faces")) {
      if (have_faces) { rc = fail(r, "contact: more than one (faces ...)"); break; }
      have_faces = 1;
      while (!rc && (t = next_token(r, buf)) == T_OPEN) {
        int k, ids[8];
        for (k = 0; (t = next_token(r, buf)) == T_ATOM; ++k) {
          if (k == 6) { rc = fail(r, "a face has at most 6 nodes"); break; }
          ids[k] = (int)strtol(buf, &end, 10);
          if (end == buf || *end) { rc = fail(r, "bad node id in a contact face"); break; }
        }
        if (rc) break;
        if (t != T_CLOSE || k == 0) { rc = fail(r, "a contact face must be a list of node ids"); break; }
        if (nfaces == 0) npf = k;
        else if (k != npf) { rc = fail(r, "every contact face must have the same number of nodes"); break; }
        if ((size_t)nfaces == cap) {
          int *q = (int *)realloc(nodes, 2 * cap * 8 * sizeof(int));
          if (!q) { rc = fail(r, "out of memory reading (contact ...)"); break; }
          nodes = q; cap *= 2;
        }
        memcpy(nodes + (size_t)nfaces * 8, ids, sizeof(int) * (size_t)k);
        nfaces++;
      }
      if (!rc && t != T_CLOSE) rc = fail(r, "(faces ...) must be a list of faces");
      continue;
    }
    {
      const int plane = ieq(buf, "plane"), sphere = ieq(buf, "sphere"), cylinder = ieq(buf, "cylinder");
      int inside = 0, have_point = 0, have_dir = 0, have_radius = 0;
      double *g;
      if (!plane && !sphere && !cylinder) { rc = fail(r, "contact: expected (faces ...), (plane ...), (sphere ...) or (cylinder ...)"); break; }
      if (nobs == FEAHIP_MAX_OBSTACLES) { rc = fail(r, "contact: more than 8 obstacles"); break; }
      g = geom + (size_t)nobs * 10;
      while (!rc) {
        t = next_token(r, buf);
        if (t == T_CLOSE) break;
        if (t != T_ATOM || buf[0] != ':') { rc = fail(r, "contact obstacle: expected :key value"); break; }
        snprintf(key, sizeof key, "%s", buf + 1);
        if (ieq(key, plane ? "point" : sphere ? "center" : "point")) { rc = read_vec3(r, g, key); have_point = 1; }
        else if (!sphere && ieq(key, plane ? "normal" : "axis")) { rc = read_vec3(r, g + 3, key); have_dir = 1; }
        else if (ieq(key, "travel")) rc = read_vec3(r, g + 7, key);
        else if (!plane && ieq(key, "radius")) {
          if (next_token(r, buf) != T_ATOM) { rc = fail(r, "attribute without a value"); break; }
          g[6] = strtod(buf, &end);
          if (end == buf || *end) { rc = fail(r, "contact: :radius is not a number"); break; }
          have_radius = 1;
        } else if (!plane && ieq(key, "inside")) {
          if (next_token(r, buf) != T_ATOM || !(ieq(buf, "t") || ieq(buf, "nil"))) { rc = fail(r, "contact: :inside must be t or nil"); break; }
          inside = ieq(buf, "t");
        } else rc = fail(r, plane ? "plane: unknown attribute (:point :normal :travel)"
                          : sphere ? "sphere: unknown attribute (:center :radius :travel :inside)"
                                   : "cylinder: unknown attribute (:point :axis :radius :travel :inside)");
      }
      if (rc) break;
      if (!have_point) { rc = fail(r, plane ? "plane needs :point" : sphere ? "sphere needs :center" : "cylinder needs :point"); break; }
      if (!sphere && !have_dir) { rc = fail(r, plane ? "plane needs :normal" : "cylinder needs :axis"); break; }
      if (!sphere && g[3] == 0 && g[4] == 0 && g[5] == 0) { rc = fail(r, plane ? "plane :normal is zero" : "cylinder :axis is zero"); break; }
      if (!plane && !have_radius) { rc = fail(r, sphere ? "sphere needs :radius" : "cylinder needs :radius"); break; }
      if (!plane && !(g[6] > 0)) { rc = fail(r, "contact: :radius must be positive"); break; }
      kind[nobs++] = plane ? FEAHIP_OBSTACLE_PLANE : sphere ? (inside ? FEAHIP_OBSTACLE_SPHERE_INSIDE : FEAHIP_OBSTACLE_SPHERE)
                                                           : (inside ? FEAHIP_OBSTACLE_CYLINDER_INSIDE : FEAHIP_OBSTACLE_CYLINDER);
    }
  }
  if (!rc && !have_penalty) rc = fail(r, "contact needs :penalty");
  if (!rc && !(penalty > 0)) rc = fail(r, "contact :penalty must be positive");
  if (!rc && (!(augment >= 0 && augment <= 2147483647.0) || augment != (double)(int)augment)) rc = fail(r, "contact :augment must be a non-negative integer");
  if (!rc && !(gap >= 0)) rc = fail(r, "contact :gap-tolerance must not be negative");
  if (!rc && nfaces == 0) rc = fail(r, "contact without (faces ...)");
  if (!rc && nobs == 0) rc = fail(r, "contact without an obstacle");
  if (rc) { free(nodes); free(kind); free(geom); return rc; }
  {
    int i;
    for (i = 0; i < nfaces; ++i) memmove(nodes + (size_t)i * npf, nodes + (size_t)i * 8, sizeof(int) * (size_t)npf);   /* pack */
  }
  free(d->contact_nodes); free(d->contact_kind); free(d->contact_geom);
  d->contact_nodes = nodes; d->contact_kind = kind; d->contact_geom = geom;
  d->contact_faces_count = nfaces; d->contact_nodes_per_face = npf; d->contact_obstacles_count = nobs;
  d->contact_penalty = penalty; d->contact_augment = (int)augment; d->contact_gap_tolerance = gap;
  return 0;
}

/* (materials (material :lambda l :mu m) ...) inside (model ...): the table of feahip_set_materials */
static int read_materials(reader *r, fea_deck *d)
{
  char buf[TOK_MAX];
  size_t n = 0;
  double *p = (double *)malloc(FEAHIP_MAX_MATERIALS * 2 * sizeof(double));   /* the largest table there is */
  int rc = 0;
  if (!p) return fail(r, "out of memory reading (materials ...)");
  for (;;) {
    attr a[ATTR_MAX];
    int na, t = next_token(r, buf);
    if (t == T_CLOSE) break;
    if (t != T_OPEN || next_token(r, buf) != T_ATOM || !ieq(buf, "material")) { rc = fail(r, "expected (material :lambda l :mu m)"); break; }
    if (n == FEAHIP_MAX_MATERIALS) { rc = fail(r, "more than 256 materials"); break; }   /* the 257th: read no further */
    if ((rc = read_attrs(r, d, a, &na, 0))) break;
    if ((rc = need_num(r, a, na, "lambda", &p[2 * n]))) break;
    if ((rc = need_num(r, a, na, "mu", &p[2 * n + 1]))) break;
    n++;
  }
  if (!rc && n == 0) rc = fail(r, "(materials ...) without a (material ...)");
  if (rc) { free(p); return rc; }
  free(d->material_params);
  d->material_params = p; d->materials_count = (int)n;
  return 0;
}

/* (element-materials i0 i1 ...) inside (geometry ...): one material id per element, deck order.  Count and range
 * are checked when the whole deck is read (the sections come in any order). */
static int read_element_materials(reader *r, fea_deck *d, int *count)
{
  char buf[TOK_MAX];
  size_t cap = 1024, n = 0;
  int *p = (int *)malloc(cap * sizeof(int)), t;
  if (!p) return fail(r, "out of memory reading (element-materials ...)");
  while ((t = next_token(r, buf)) == T_ATOM) {
    char *end;
    if (n == cap) {
      int *q = (int *)realloc(p, 2 * cap * sizeof(int));
      if (!q) { free(p); return fail(r, "out of memory reading (element-materials ...)"); }
      p = q; cap *= 2;
    }
    p[n] = (int)strtol(buf, &end, 10);
    if (end == buf || *end) { free(p); return fail(r, "bad material id in element-materials"); }
    n++;
  }
  if (t != T_CLOSE) { free(p); return fail(r, "element-materials must be a flat list of material ids"); }
  free(d->element_material);
  d->element_material = p; *count = (int)n;
  return 0;
}

/* (points (f v) ...) of (spectrum ...) and (psd (f v) ...) of (random ...): pairs of numbers, f strictly ascending and not
 * negative, v not negative, all finite */
static int read_pairs(reader *r, double **out, int *count, const char *what)
{
  char buf[TOK_MAX], m[96];
  size_t cap = 64, n = 0;
  double *p = (double *)malloc(cap * 2 * sizeof(double));
  int t, k;
  if (!p) return fail(r, "out of memory reading a list of points");
  while ((t = next_token(r, buf)) == T_OPEN) {
    if (n == FEA_DECK_MAX_POINTS) { free(p); snprintf(m, sizeof m, "%s: more than %d points", what, FEA_DECK_MAX_POINTS); return fail(r, m); }
    if (n == cap) {
      double *q = (double *)realloc(p, 2 * cap * 2 * sizeof(double));
      if (!q) { free(p); return fail(r, "out of memory reading a list of points"); }
      p = q; cap *= 2;
    }
    for (k = 0; k < 2; ++k) {
      char *end;
      double v;
      if (next_token(r, buf) != T_ATOM) { free(p); snprintf(m, sizeof m, "%s: a point is a pair of numbers", what); return fail(r, m); }
      v = strtod(buf, &end);
      if (end == buf || *end || !(v >= 0 && v <= 1.7976931348623157e308)) {
        free(p); snprintf(m, sizeof m, "%s: the numbers of a point must be finite and not negative", what); return fail(r, m);
      }
      p[2 * n + k] = v;
    }
    if (next_token(r, buf) != T_CLOSE) { free(p); snprintf(m, sizeof m, "%s: a point is a pair of numbers", what); return fail(r, m); }
    if (n > 0 && !(p[2 * n] > p[2 * n - 2])) { free(p); snprintf(m, sizeof m, "%s: the frequencies must be strictly ascending", what); return fail(r, m); }
    n++;
  }
  if (t != T_CLOSE) { free(p); snprintf(m, sizeof m, "%s: expected a list of (f value) pairs", what); return fail(r, m); }
  free(*out);
  *out = p; *count = (int)n;
  return 0;
}

/* t or nil; the value given stays where the attribute is absent */
static int read_flag(reader *r, const attr *a, int na, const char *key, int *flag, const char *msg)
{
  const char *s = attr_get(a, na, key);
  if (!s) return 0;
  if (ieq(s, "nil") || ieq(s, "no") || ieq(s, "false")) *flag = 0;
  else if (ieq(s, "t") || ieq(s, "yes") || ieq(s, "true")) *flag = 1;
  else return fail(r, msg);
  return 0;
}

/* :base (bx by bz), its atoms blank-separated by read_attrs: three finite numbers, not all zero */
static int read_base(reader *r, const attr *a, int na, int *has, double *base, const char *msg)
{
  const char *s = attr_get(a, na, "base");
  char *end;
  int k;
  *has = 0; base[0] = base[1] = base[2] = 0;
  if (!s) return 0;
  for (k = 0; k < 3; ++k) {
    base[k] = strtod(s, &end);
    if (end == s || !(base[k] >= -1.7976931348623157e308 && base[k] <= 1.7976931348623157e308)) return fail(r, msg);
    s = end;
  }
  while (*s == ' ') ++s;
  if (*s || (base[0] == 0 && base[1] == 0 && base[2] == 0)) return fail(r, msg);
  *has = 1;
  return 0;
}

/* one list, '(' consumed: dispatch on the head like traverse_function
 * (sexp_loader.c:249-272) */
static int read_list(reader *r, fea_deck *d)
{
  char head[TOK_MAX];
  attr a[ATTR_MAX];
  int na, t = next_token(r, head);
  double v;
  const char *s;
  if (t == T_CLOSE) return 0;
  if (t == T_OPEN) {                     /* list of lists */
    if (read_list(r, d)) return -1;
    head[0] = 0;
  } else if (t == T_EOF)
    return fail(r, "unexpected end of file");

  if (ieq(head, "nodes")) return read_nodes(r, d);
  if (ieq(head, "elements")) return read_elements(r, d);
  if (ieq(head, "prescribed-displacements")) return read_prescribed(r, d);
  if (ieq(head, "surface-loads")) return read_surface(r, d);
  if (ieq(head, "contact")) return read_contact(r, d);
  if (ieq(head, "materials")) return read_materials(r, d);
  if (ieq(head, "element-materials")) return read_element_materials(r, d, &r->n_element_material);
  if (ieq(head, "points")) return read_pairs(r, &d->spectrum_points, &d->spectrum_count, "spectrum (points ...)");
  if (ieq(head, "psd")) return read_pairs(r, &d->random_points, &d->random_count, "random (psd ...)");

  if (read_attrs(r, d, a, &na, 1)) return -1;
  if (attr_get(a, na, "stress") && !ieq(head, "spectrum") && !ieq(head, "random") && !ieq(head, "harmonic") && !ieq(head, "transient"))
    return fail(r, ":stress belongs to (harmonic ...), (transient ...), (spectrum ...) and (random ...)");

  if (ieq(head, "model")) {                                   /* :32-54 */
    if ((s = attr_get(a, na, "name"))) {
      if (ieq(s, "A5")) { d->model = FEAHIP_MODEL_A5; d->parameters_count = 2; }
      else if (ieq(s, "COMPRESSIBLE_NEOHOOKEAN")) { d->model = FEAHIP_MODEL_COMPRESSIBLE_NEOHOOKEAN; d->parameters_count = 2; }
      else { char m[TOK_MAX + 32]; snprintf(m, sizeof m, "unknown model type '%s'", s); return fail(r, m); }
    }
  } else if (ieq(head, "model-parameters")) {                 /* :56-73 */
    if (need_num(r, a, na, "lambda", &d->parameters[0])) return -1;
    if (need_num(r, a, na, "mu", &d->parameters[1])) return -1;
  } else if (ieq(head, "solution")) {                         /* :75-95 */
    if (need_num(r, a, na, "desired-tolerance", &d->desired_tolerance)) return -1;
    if (!attr_get(a, na, "task-type")) return fail(r, "missing attribute :task-type");
    if (need_num(r, a, na, "load-increments-count", &v)) return -1;
    d->load_increments_count = (int)v;
    if (!(s = attr_get(a, na, "modified-newton"))) return fail(r, "missing attribute :modified-newton");
    d->modified_newton = (ieq(s, "YES") || ieq(s, "TRUE")) ? 1 : 0;
    if (need_num(r, a, na, "max-newton-count", &v)) return -1;
    d->max_newton_count = (int)v;
  } else if (ieq(head, "slae-solver")) {                      /* :97-138 */
    d->solver_type = FEAHIP_CG; d->solver_tolerance = 1e-14; d->solver_max_iter = 20000;
    if ((s = attr_get(a, na, "type"))) {
      if (ieq(s, "CG") || ieq(s, "PCG_ILU")) {
        d->solver_type = ieq(s, "CG") ? FEAHIP_CG : FEAHIP_PCG_ILU;
        if (attr_get(a, na, "tolerance") && need_num(r, a, na, "tolerance", &d->solver_tolerance)) return -1;
        if (attr_get(a, na, "max-iterations")) {
          if (need_num(r, a, na, "max-iterations", &v)) return -1;
          d->solver_max_iter = (int)v;
        }
      } else if (ieq(s, "CHOLESKY")) d->solver_type = FEAHIP_CHOLESKY;
      else { char m[TOK_MAX + 32]; snprintf(m, sizeof m, "unknown solver type '%s'", s); return fail(r, m); }
    }
  } else if (ieq(head, "element-type")) {                     /* :141-155 */
    if (need_num(r, a, na, "gauss-nodes-count", &v)) return -1;
    d->gauss_nodes_count = (int)v;
    if (need_num(r, a, na, "nodes-count", &v)) return -1;
    d->nodes_per_element = (int)v;
    if (!(s = attr_get(a, na, "name"))) return fail(r, "missing attribute :name");
    if (ieq(s, "TETRAHEDRA10")) d->ele_type = FEA_TETRAHEDRA10;
    else if (ieq(s, "TETRAHEDRA4")) d->ele_type = FEA_TETRAHEDRA4;   /* build extension */
    else if (ieq(s, "HEXAHEDRA8")) d->ele_type = FEA_HEXAHEDRA8;     /* build extension */
    else { char m[TOK_MAX + 32]; snprintf(m, sizeof m, "unknown element type '%s'", s); return fail(r, m); }
  } else if (ieq(head, "line-search")) {                      /* :157-163 */
    if (need_num(r, a, na, "max", &v)) return -1;
    d->linesearch_max = (int)v;
  } else if (ieq(head, "arc-length")) {                       /* :165-171 */
    if (need_num(r, a, na, "max", &v)) return -1;
    d->arclength_max = (int)v;
  } else if (ieq(head, "dynamics")) {                         /* no counterpart in the reference */
    if (need_num(r, a, na, "steps", &v)) return -1;
    if (!(v >= 0 && v <= 2147483647.0) || v != (double)(int)v) return fail(r, "dynamics :steps must be a non-negative integer");
    d->dynamics_steps = (int)v;
    if (need_num(r, a, na, "dt", &d->dynamics_dt)) return -1;
    d->dynamics_explicit = 0; d->dynamics_safety = 0.9; d->dynamics_restep = 0;
    if (attr_get(a, na, "scheme")) {
      const char *sc = attr_get(a, na, "scheme");
      if (ieq(sc, "explicit")) d->dynamics_explicit = 1;
      else if (!ieq(sc, "newmark")) return fail(r, "dynamics :scheme must be newmark or explicit");
    }
    if (!d->dynamics_explicit && (attr_get(a, na, "safety") || attr_get(a, na, "restep")))
      return fail(r, "dynamics :safety and :restep need :scheme explicit");
    if (d->dynamics_explicit) {
      if (attr_get(a, na, "safety") && need_num(r, a, na, "safety", &d->dynamics_safety)) return -1;
      if (!(d->dynamics_safety > 0 && d->dynamics_safety <= 1)) return fail(r, "dynamics :safety must be in (0, 1]");
      if (attr_get(a, na, "restep")) {
        if (need_num(r, a, na, "restep", &v)) return -1;
        if (!(v >= 0 && v <= 2147483647.0) || v != (double)(int)v) return fail(r, "dynamics :restep must be a non-negative integer");
        d->dynamics_restep = (int)v;
      }
      if (!(d->dynamics_dt >= 0)) return fail(r, "dynamics :dt must not be negative");
    } else if (!(d->dynamics_dt > 0)) return fail(r, "dynamics :dt must be positive");
    d->dynamics_beta = 0.25; d->dynamics_gamma = 0.5; d->dynamics_dlambda = 0;
    if (attr_get(a, na, "beta") && need_num(r, a, na, "beta", &d->dynamics_beta)) return -1;
    if (attr_get(a, na, "gamma") && need_num(r, a, na, "gamma", &d->dynamics_gamma)) return -1;
    if (attr_get(a, na, "dlambda") && need_num(r, a, na, "dlambda", &d->dynamics_dlambda)) return -1;
    if (!(d->dynamics_beta > 0)) return fail(r, "dynamics :beta must be positive");
    if (!(d->dynamics_gamma >= 0)) return fail(r, "dynamics :gamma must not be negative");
    if (need_num(r, a, na, "density", &d->density)) return -1;
    if (!(d->density > 0)) return fail(r, "dynamics :density must be positive");
    d->damping_alpha = d->damping_beta = 0;
    if (attr_get(a, na, "damping-alpha") && need_num(r, a, na, "damping-alpha", &d->damping_alpha)) return -1;
    if (attr_get(a, na, "damping-beta") && need_num(r, a, na, "damping-beta", &d->damping_beta)) return -1;
    if (!(d->damping_alpha >= 0 && d->damping_alpha < HUGE_VAL) || !(d->damping_beta >= 0 && d->damping_beta < HUGE_VAL))
      return fail(r, "dynamics :damping-alpha and :damping-beta must be finite and not negative");
    if (d->dynamics_explicit && d->damping_beta != 0)
      return fail(r, "dynamics :scheme explicit takes mass-proportional damping only: :damping-beta must be 0");
    d->has_dynamics = 1;
  } else if (ieq(head, "results")) {                          /* no counterpart in the reference */
    static const char *key[3] = {"nodal-stress", "energy", "reactions"};
    int *flag[3], i;
    flag[0] = &d->results_nodal_stress; flag[1] = &d->results_energy; flag[2] = &d->results_reactions;
    for (i = 0; i < 3; ++i) {
      *flag[i] = 0;
      if ((s = attr_get(a, na, key[i]))) {
        if (ieq(s, "t") || ieq(s, "yes") || ieq(s, "true")) *flag[i] = 1;
        else if (!(ieq(s, "nil") || ieq(s, "no") || ieq(s, "false"))) return fail(r, "results attributes take t or nil");
      }
    }
  } else if (ieq(head, "modal")) {                            /* no counterpart in the reference */
    d->modal_modes = d->modal_count = 0; d->modal_shift = 0.0;
    if (attr_get(a, na, "count")) {                           /* :count N, up to 64 modes by the locked solve, instead of :modes */
      if (attr_get(a, na, "modes")) return fail(r, "modal takes :modes or :count, not both");
      if (need_num(r, a, na, "count", &v)) return -1;
      if (!(v >= 1 && v <= FEA_MODAL_MAX_LOCKED) || v != (double)(int)v) return fail(r, "modal :count must be an integer in [1, 64]");
      d->modal_count = (int)v;
    } else {
      if (need_num(r, a, na, "modes", &v)) return -1;
      if (!(v >= 0 && v <= FEA_MODAL_COLS) || v != (double)(int)v) return fail(r, "modal :modes must be an integer in [0, 8]");
      d->modal_modes = (int)v;
    }
    if (attr_get(a, na, "shift")) {
      if (need_num(r, a, na, "shift", &d->modal_shift)) return -1;
      if (!(d->modal_shift >= 0 && d->modal_shift <= 1.7976931348623157e308)) return fail(r, "modal :shift must be finite and not negative");
    }
    d->modal_tolerance = 1e-8; d->modal_max = 1000;
    if (attr_get(a, na, "tolerance") && need_num(r, a, na, "tolerance", &d->modal_tolerance)) return -1;
    if (!(d->modal_tolerance > 0)) return fail(r, "modal :tolerance must be positive");
    if (attr_get(a, na, "max")) {
      if (need_num(r, a, na, "max", &v)) return -1;
      if (!(v >= 0 && v <= 2147483647.0) || v != (double)(int)v) return fail(r, "modal :max must be a non-negative integer");
      d->modal_max = (int)v;
    }
  } else if (ieq(head, "harmonic")) {                         /* no counterpart in the reference */
    if (need_num(r, a, na, "count", &v)) return -1;
    if (!(v >= 1 && v <= FEA_RESPONSE_MAX_FREQ) || v != (double)(int)v) return fail(r, "harmonic :count must be an integer in [1, 4096]");
    d->harmonic_count = (int)v;
    if (need_num(r, a, na, "from", &d->harmonic_from)) return -1;
    if (need_num(r, a, na, "to", &d->harmonic_to)) return -1;
    if (!(d->harmonic_from >= 0 && d->harmonic_from <= d->harmonic_to && d->harmonic_to <= 1.7976931348623157e308))
      return fail(r, "harmonic needs 0 <= :from <= :to, both finite");
    d->harmonic_zeta = 0; d->harmonic_static = 1;
    if (attr_get(a, na, "zeta") && need_num(r, a, na, "zeta", &d->harmonic_zeta)) return -1;
    if (!(d->harmonic_zeta >= 0 && d->harmonic_zeta <= 1.7976931348623157e308)) return fail(r, "harmonic :zeta must be finite and not negative");
    if ((s = attr_get(a, na, "static-correction"))) {
      if (ieq(s, "nil") || ieq(s, "no") || ieq(s, "false")) d->harmonic_static = 0;
      else if (!(ieq(s, "t") || ieq(s, "yes") || ieq(s, "true"))) return fail(r, "harmonic :static-correction takes t or nil");
    }
    d->harmonic_stress = 0;
    if (read_flag(r, a, na, "stress", &d->harmonic_stress, "harmonic :stress takes t or nil")) return -1;
  } else if (ieq(head, "transient")) {                        /* no counterpart in the reference */
    if (need_num(r, a, na, "steps", &v)) return -1;
    if (!(v >= 1 && v <= FEA_TRANSIENT_MAX_STEPS) || v != (double)(int)v) return fail(r, "transient :steps must be an integer in [1, 1048576]");
    d->transient_steps = (int)v;
    if (need_num(r, a, na, "dt", &d->transient_dt)) return -1;
    if (!(d->transient_dt > 0 && d->transient_dt <= 1.7976931348623157e308)) return fail(r, "transient :dt must be positive and finite");
    d->transient_zeta = 0; d->transient_static = 1; d->transient_shape = FEA_SHAPE_STEP; d->transient_rise = 0;
    d->transient_has_base = 0; d->transient_base[0] = d->transient_base[1] = d->transient_base[2] = 0;
    if (attr_get(a, na, "zeta") && need_num(r, a, na, "zeta", &d->transient_zeta)) return -1;
    if (!(d->transient_zeta >= 0 && d->transient_zeta <= 1.7976931348623157e308)) return fail(r, "transient :zeta must be finite and not negative");
    if ((s = attr_get(a, na, "static-correction"))) {
      if (ieq(s, "nil") || ieq(s, "no") || ieq(s, "false")) d->transient_static = 0;
      else if (!(ieq(s, "t") || ieq(s, "yes") || ieq(s, "true"))) return fail(r, "transient :static-correction takes t or nil");
    }
    if ((s = attr_get(a, na, "shape"))) {
      if (ieq(s, "step")) d->transient_shape = FEA_SHAPE_STEP;
      else if (ieq(s, "ramp")) d->transient_shape = FEA_SHAPE_RAMP;
      else if (ieq(s, "half-sine")) d->transient_shape = FEA_SHAPE_HALF_SINE;
      else return fail(r, "transient :shape must be step, ramp or half-sine");
    }
    if (attr_get(a, na, "rise") && need_num(r, a, na, "rise", &d->transient_rise)) return -1;
    if (d->transient_shape != FEA_SHAPE_STEP && !(d->transient_rise > 0 && d->transient_rise <= 1.7976931348623157e308))
      return fail(r, "transient :rise must be positive and finite for a ramp or a half-sine");
    if ((s = attr_get(a, na, "base"))) {
      char *end;
      int k;
      for (k = 0; k < 3; ++k) {
        d->transient_base[k] = strtod(s, &end);
        if (end == s || !(d->transient_base[k] >= -1.7976931348623157e308 && d->transient_base[k] <= 1.7976931348623157e308))
          return fail(r, "transient :base takes three finite numbers");
        s = end;
      }
      while (*s == ' ') ++s;
      if (*s) return fail(r, "transient :base takes three finite numbers");
      if (d->transient_base[0] == 0 && d->transient_base[1] == 0 && d->transient_base[2] == 0) return fail(r, "transient :base must not be zero");
      d->transient_has_base = 1;
    }
    d->transient_stress = 0;
    if (read_flag(r, a, na, "stress", &d->transient_stress, "transient :stress takes t or nil")) return -1;
    d->transient_sn_exponent = d->transient_sn_coefficient = 0; d->transient_rainflow_depth = 32;
    if (attr_get(a, na, "sn-exponent")) {
      if (!d->transient_stress) return fail(r, "transient :sn-exponent needs :stress t");
      if (need_num(r, a, na, "sn-exponent", &d->transient_sn_exponent)) return -1;
      if (!(d->transient_sn_exponent >= 1 && d->transient_sn_exponent <= 64)) return fail(r, "transient :sn-exponent must be in [1, 64]");
      if (need_num(r, a, na, "sn-coefficient", &d->transient_sn_coefficient)) return -1;
      if (!(d->transient_sn_coefficient > 0 && d->transient_sn_coefficient <= 1.7976931348623157e308)) return fail(r, "transient :sn-coefficient must be positive and finite");
      if (attr_get(a, na, "rainflow-depth")) {
        if (need_num(r, a, na, "rainflow-depth", &v)) return -1;
        if (!(v >= 4 && v <= FEA_RAINFLOW_MAX_DEPTH) || v != (double)(int)v) return fail(r, "transient :rainflow-depth must be an integer in [4, 1024]");
        d->transient_rainflow_depth = (int)v;
      }
    } else if (attr_get(a, na, "sn-coefficient") || attr_get(a, na, "rainflow-depth"))
      return fail(r, "transient :sn-coefficient and :rainflow-depth need :sn-exponent");
  } else if (ieq(head, "spectrum")) {                         /* no counterpart in the reference */
    d->spectrum_rule = FEAHIP_SRSS; d->spectrum_zeta = 0; d->spectrum_zpa = 0; d->spectrum_static = 1; d->spectrum_loglog = 0;
    if ((s = attr_get(a, na, "rule"))) {
      if (ieq(s, "srss")) d->spectrum_rule = FEAHIP_SRSS;
      else if (ieq(s, "cqc")) d->spectrum_rule = FEAHIP_CQC;
      else if (ieq(s, "abs")) d->spectrum_rule = FEAHIP_ABS;
      else return fail(r, "spectrum :rule must be srss, cqc or abs");
    }
    if (attr_get(a, na, "zeta") && need_num(r, a, na, "zeta", &d->spectrum_zeta)) return -1;
    if (!(d->spectrum_zeta >= 0 && d->spectrum_zeta <= 1.7976931348623157e308)) return fail(r, "spectrum :zeta must be finite and not negative");
    if (attr_get(a, na, "zpa") && need_num(r, a, na, "zpa", &d->spectrum_zpa)) return -1;
    if (!(d->spectrum_zpa >= 0 && d->spectrum_zpa <= 1.7976931348623157e308)) return fail(r, "spectrum :zpa must be finite and not negative");
    if (read_flag(r, a, na, "static-correction", &d->spectrum_static, "spectrum :static-correction takes t or nil")) return -1;
    if ((s = attr_get(a, na, "interp"))) {
      if (ieq(s, "loglog")) d->spectrum_loglog = 1;
      else if (!ieq(s, "linear")) return fail(r, "spectrum :interp must be linear or loglog");
    }
    if (read_base(r, a, na, &d->spectrum_has_base, d->spectrum_base, "spectrum :base takes three finite numbers, not all zero")) return -1;
    if (d->spectrum_zpa > 0 && !d->spectrum_static) return fail(r, "spectrum :zpa needs :static-correction t");
    if (d->spectrum_zpa > 0 && d->spectrum_rule == FEAHIP_ABS) return fail(r, "spectrum :zpa needs a rule other than abs");
    d->spectrum_stress = 0;
    if (read_flag(r, a, na, "stress", &d->spectrum_stress, "spectrum :stress takes t or nil")) return -1;
    if (d->spectrum_stress && d->spectrum_rule == FEAHIP_ABS) return fail(r, "spectrum :stress needs a rule other than abs");
    if (d->spectrum_count < 1) return fail(r, "spectrum needs (points (f sa) ...)");
    d->has_spectrum = 1;
  } else if (ieq(head, "random")) {                           /* no counterpart in the reference */
    d->random_zeta = 0; d->random_static = 1; d->random_loglog = 0; d->random_per_mode = 32; d->random_background = 257;
    if (attr_get(a, na, "zeta") && need_num(r, a, na, "zeta", &d->random_zeta)) return -1;
    if (!(d->random_zeta >= 0 && d->random_zeta <= 1.7976931348623157e308)) return fail(r, "random :zeta must be finite and not negative");
    if (read_flag(r, a, na, "static-correction", &d->random_static, "random :static-correction takes t or nil")) return -1;
    if ((s = attr_get(a, na, "interp"))) {
      if (ieq(s, "loglog")) d->random_loglog = 1;
      else if (!ieq(s, "linear")) return fail(r, "random :interp must be linear or loglog");
    }
    if (attr_get(a, na, "per-mode")) {
      if (need_num(r, a, na, "per-mode", &v)) return -1;
      if (!(v >= 0 && v <= 4096) || v != (double)(int)v) return fail(r, "random :per-mode must be an integer in [0, 4096]");
      d->random_per_mode = (int)v;
    }
    if (attr_get(a, na, "background")) {
      if (need_num(r, a, na, "background", &v)) return -1;
      if (!(v >= 2 && v <= 131072) || v != (double)(int)v) return fail(r, "random :background must be an integer in [2, 131072]");
      d->random_background = (int)v;
    }
    if (read_base(r, a, na, &d->random_has_base, d->random_base, "random :base takes three finite numbers, not all zero")) return -1;
    d->random_stress = 0;
    if (read_flag(r, a, na, "stress", &d->random_stress, "random :stress takes t or nil")) return -1;
    d->random_sn_exponent = d->random_sn_coefficient = 0; d->random_duration = 1;
    if (attr_get(a, na, "sn-exponent")) {
      if (need_num(r, a, na, "sn-exponent", &d->random_sn_exponent)) return -1;
      if (!(d->random_sn_exponent >= 1 && d->random_sn_exponent <= 64)) return fail(r, "random :sn-exponent must be in [1, 64]");
      if (need_num(r, a, na, "sn-coefficient", &d->random_sn_coefficient)) return -1;
      if (!(d->random_sn_coefficient > 0 && d->random_sn_coefficient <= 1.7976931348623157e308)) return fail(r, "random :sn-coefficient must be positive and finite");
      if (attr_get(a, na, "duration") && need_num(r, a, na, "duration", &d->random_duration)) return -1;
      if (!(d->random_duration > 0 && d->random_duration <= 1.7976931348623157e308)) return fail(r, "random :duration must be positive and finite");
    } else if (attr_get(a, na, "sn-coefficient") || attr_get(a, na, "duration"))
      return fail(r, "random :sn-coefficient and :duration need :sn-exponent");
    if (d->random_count < 2) return fail(r, "random needs (psd (f s) ...) with two points at least");
    d->has_random = 1;
  } else if (ieq(head, "buckling")) {                         /* no counterpart in the reference */
    if (need_num(r, a, na, "modes", &v)) return -1;
    if (!(v >= 1 && v <= FEA_MODAL_COLS) || v != (double)(int)v) return fail(r, "buckling :modes must be an integer in [1, 8]");
    d->buckling_modes = (int)v;
    d->buckling_tolerance = 1e-8; d->buckling_max = 2000;
    if (attr_get(a, na, "tolerance") && need_num(r, a, na, "tolerance", &d->buckling_tolerance)) return -1;
    if (!(d->buckling_tolerance > 0 && d->buckling_tolerance <= 1.7976931348623157e308)) return fail(r, "buckling :tolerance must be positive");
    if (attr_get(a, na, "max")) {
      if (need_num(r, a, na, "max", &v)) return -1;
      if (!(v >= 0 && v <= 2147483647.0) || v != (double)(int)v) return fail(r, "buckling :max must be a non-negative integer");
      d->buckling_max = (int)v;
    }
  } else if (ieq(head, "body-force")) {
    if (need_num(r, a, na, "x", &d->body_force[0])) return -1;
    if (need_num(r, a, na, "y", &d->body_force[1])) return -1;
    if (need_num(r, a, na, "z", &d->body_force[2])) return -1;
    d->has_body_force = 1;
  }
  return 0;
}

static void deck_defaults(fea_deck *d)
{
  memset(d, 0, sizeof(*d));
  d->desired_tolerance = 1e-8;                 /* fea_solver.c:1514-1527 */
  d->ele_type = FEA_TETRAHEDRA10;
  d->modified_newton = 1;
  d->model = FEAHIP_MODEL_A5;
  d->parameters_count = 2;
  d->parameters[0] = 100; d->parameters[1] = 100;
  d->gauss_nodes_count = 5;                    /* :1546-1547 */
  d->nodes_per_element = 10;
  d->solver_type = FEAHIP_CG;                  /* sexp_loader.c:101-103 */
  d->solver_tolerance = 1e-14;
  d->solver_max_iter = 20000;
}

int fea_deck_load(const char *path, fea_deck *deck, char *errbuf, int errlen)
{
  reader r;
  char buf[TOK_MAX];
  int t, rc;
  deck_defaults(deck);
  r.line = 1; r.err[0] = 0; r.n_element_material = -1;
  r.f = fopen(path, "rt");
  if (!r.f) {
    if (errbuf) snprintf(errbuf, (size_t)errlen, "could not open file %s", path);
    return -1;
  }
  t = next_token(&r, buf);
  if (t != T_OPEN || next_token(&r, buf) != T_ATOM || !ieq(buf, "task")) {
    fclose(r.f);
    if (errbuf) snprintf(errbuf, (size_t)errlen, "deck does not start with (task");
    return -1;
  }
  {
    attr a[ATTR_MAX];
    int na;
    rc = read_attrs(&r, deck, a, &na, 1);
  }
  fclose(r.f);
  if (rc == 0) {
    int i;
    if (deck->nodes_count == 0 || deck->elements_count == 0) { rc = -1; snprintf(r.err, sizeof r.err, "deck has no nodes or no elements"); }
    for (i = 0; rc == 0 && i < deck->elements_count * deck->nodes_per_element; ++i)
      if (deck->elements[i] < 0 || deck->elements[i] >= deck->nodes_count) {
        rc = -1; snprintf(r.err, sizeof r.err, "element %d refers to node %d outside the node list", i / deck->nodes_per_element, deck->elements[i]);
      }
    /* the material table: both sections or neither, one id per element, every id a row of the table */
    if (rc == 0 && (deck->materials_count > 0) != (r.n_element_material >= 0)) {
      rc = -1;
      snprintf(r.err, sizeof r.err, deck->materials_count > 0 ? "deck has (materials ...) but no (element-materials ...)"
                                                               : "deck has (element-materials ...) but no (materials ...)");
    }
    if (rc == 0 && deck->materials_count > 0 && r.n_element_material != deck->elements_count) {
      rc = -1; snprintf(r.err, sizeof r.err, "element-materials has %d ids for %d elements", r.n_element_material, deck->elements_count);
    }
    for (i = 0; rc == 0 && deck->materials_count > 0 && i < deck->elements_count; ++i)
      if (deck->element_material[i] < 0 || deck->element_material[i] >= deck->materials_count) {
        rc = -1; snprintf(r.err, sizeof r.err, "element %d has material %d outside [0,%d)", i, deck->element_material[i], deck->materials_count);
      }
    if (rc == 0 && deck->has_body_force && !deck->has_dynamics) {
      rc = -1; snprintf(r.err, sizeof r.err, "deck has (body-force ...) but no (dynamics ... :density rho)");
    }
    if (rc == 0 && (deck->modal_modes > 0 || deck->modal_count > 0) && !deck->has_dynamics) {
      rc = -1; snprintf(r.err, sizeof r.err, "deck has (modal ...) but no density: add (dynamics :steps 0 :dt 1 :density rho)");
    }
    if (rc == 0 && deck->harmonic_count > 0 && !(deck->modal_count > 0 || (deck->modal_modes > 0 && deck->modal_shift != 0.0))) {
      rc = -1; snprintf(r.err, sizeof r.err, "deck has (harmonic ...) but no locked modes: add (modal :count N ...) or a :shift");
    }
    if (rc == 0 && deck->transient_steps > 0 && !(deck->modal_count > 0 || (deck->modal_modes > 0 && deck->modal_shift != 0.0))) {
      rc = -1; snprintf(r.err, sizeof r.err, "deck has (transient ...) but no locked modes: add (modal :count N ...) or a :shift");
    }
    if (rc == 0 && (deck->has_spectrum || deck->has_random) && !(deck->modal_count > 0 || (deck->modal_modes > 0 && deck->modal_shift != 0.0))) {
      rc = -1; snprintf(r.err, sizeof r.err, "deck has (%s ...) but no locked modes: add (modal :count N ...) or a :shift", deck->has_spectrum ? "spectrum" : "random");
    }
    if (rc == 0 && deck->has_spectrum && deck->spectrum_static && deck->modal_shift != 0.0) {
      rc = -1; snprintf(r.err, sizeof r.err, "spectrum :static-correction t and a non-zero modal :shift exclude each other");
    }
    if (rc == 0 && deck->has_random && deck->random_static && deck->modal_shift != 0.0) {
      rc = -1; snprintf(r.err, sizeof r.err, "random :static-correction t and a non-zero modal :shift exclude each other");
    }
    if (rc == 0 && deck->transient_steps > 0 && deck->transient_static && deck->modal_shift != 0.0) {
      rc = -1; snprintf(r.err, sizeof r.err, "transient :static-correction t and a non-zero modal :shift exclude each other");
    }
    if (rc == 0 && deck->harmonic_count > 0 && deck->harmonic_static && deck->modal_shift != 0.0) {
      rc = -1; snprintf(r.err, sizeof r.err, "harmonic :static-correction t and a non-zero modal :shift exclude each other");
    }
  }
  if (rc) {
    if (errbuf) snprintf(errbuf, (size_t)errlen, "%s", r.err);
    fea_deck_free(deck);
    return -1;
  }
  return 0;
}

void fea_deck_free(fea_deck *d)
{
  if (!d) return;
  free(d->nodes); free(d->elements);
  free(d->presc_node); free(d->presc_type); free(d->presc_values);
  free(d->surface_nodes); free(d->surface_kind); free(d->surface_values);
  free(d->contact_nodes); free(d->contact_kind); free(d->contact_geom);
  d->contact_nodes = d->contact_kind = NULL; d->contact_geom = NULL;
  d->contact_faces_count = d->contact_obstacles_count = 0;
  free(d->spectrum_points); free(d->random_points);
  d->spectrum_points = d->random_points = NULL; d->spectrum_count = d->random_count = d->has_spectrum = d->has_random = 0;
  d->spectrum_stress = d->random_stress = d->harmonic_stress = d->transient_stress = 0;
  d->random_sn_exponent = d->random_sn_coefficient = d->random_duration = 0;
  d->transient_sn_exponent = d->transient_sn_coefficient = 0; d->transient_rainflow_depth = 0;
  free(d->material_params); free(d->element_material);
  d->material_params = NULL; d->element_material = NULL; d->materials_count = 0;
  d->nodes = NULL; d->elements = NULL;
  d->presc_node = d->presc_type = NULL; d->presc_values = NULL;
  d->surface_nodes = d->surface_kind = NULL; d->surface_values = NULL;
  d->nodes_count = d->elements_count = d->prescribed_nodes_count = d->surface_faces_count = 0;
}

int fea_deck_save(const char *path, const fea_deck *d)
{
  static const char *solver[] = {"CG", "PCG_ILU", "CHOLESKY"};
  FILE *f = fopen(path, "wt");
  int i, k;
  if (!f) return -1;
  fprintf(f, ";; -*- Mode: lisp; -*-\n(task\n");
  fprintf(f, " (model :name %s\n        (model-parameters :mu %.17g :lambda %.17g)",
          d->model == FEAHIP_MODEL_A5 ? "A5" : "COMPRESSIBLE_NEOHOOKEAN", d->parameters[1], d->parameters[0]);
  if (d->materials_count > 0) {                      /* written only when there is a table: other decks save as before */
    fprintf(f, "\n        (materials");
    for (i = 0; i < d->materials_count; ++i)
      fprintf(f, "\n         (material :lambda %.17g :mu %.17g)", d->material_params[2 * i], d->material_params[2 * i + 1]);
    fprintf(f, ")");
  }
  fprintf(f, ")\n");
  fprintf(f, " (solution :desired-tolerance %.17g :task-type CARTESIAN3D :load-increments-count %d"
             " :modified-newton %s :max-newton-count %d\n",
          d->desired_tolerance, d->load_increments_count, d->modified_newton ? "yes" : "no", d->max_newton_count);
  fprintf(f, "   (element-type :gauss-nodes-count %d :name %s :nodes-count %d)\n", d->gauss_nodes_count,
          d->ele_type == FEA_TETRAHEDRA4 ? "TETRAHEDRA4" : d->ele_type == FEA_HEXAHEDRA8 ? "HEXAHEDRA8" : "TETRAHEDRA10", d->nodes_per_element);
  fprintf(f, "   (slae-solver :type %s :tolerance %.17g :max-iterations %d)\n", solver[d->solver_type],
          d->solver_tolerance, d->solver_max_iter);
  fprintf(f, "   (line-search :max %d)\n   (arc-length :max %d)", d->linesearch_max, d->arclength_max);
  if (d->has_dynamics)                               /* written only when present: other decks save as before */
    fprintf(f, "\n   (dynamics :steps %d :dt %.17g :beta %.17g :gamma %.17g :dlambda %.17g :density %.17g", d->dynamics_steps,
            d->dynamics_dt, d->dynamics_beta, d->dynamics_gamma, d->dynamics_dlambda, d->density);
  if (d->has_dynamics && d->dynamics_explicit)
    fprintf(f, " :scheme explicit :safety %.17g :restep %d", d->dynamics_safety, d->dynamics_restep);
  if (d->has_dynamics && d->damping_alpha != 0) fprintf(f, " :damping-alpha %.17g", d->damping_alpha);
  if (d->has_dynamics && d->damping_beta != 0) fprintf(f, " :damping-beta %.17g", d->damping_beta);
  if (d->has_dynamics) fprintf(f, ")");
  if (d->results_nodal_stress || d->results_energy || d->results_reactions)   /* written only when asked for */
    fprintf(f, "\n   (results :nodal-stress %s :energy %s :reactions %s)", d->results_nodal_stress ? "t" : "nil",
            d->results_energy ? "t" : "nil", d->results_reactions ? "t" : "nil");
  if (d->modal_modes > 0 || d->modal_count > 0) {                              /* written only when asked for */
    fprintf(f, "\n   (modal :%s %d :tolerance %.17g :max %d", d->modal_count > 0 ? "count" : "modes",
            d->modal_count > 0 ? d->modal_count : d->modal_modes, d->modal_tolerance, d->modal_max);
    if (d->modal_shift != 0.0) fprintf(f, " :shift %.17g", d->modal_shift);    /* (the old text without the new keys) */
    fprintf(f, ")");
  }
  if (d->harmonic_count > 0) {                                                 /* written only when asked for */
    fprintf(f, "\n   (harmonic :from %.17g :to %.17g :count %d :zeta %.17g :static-correction %s", d->harmonic_from,
            d->harmonic_to, d->harmonic_count, d->harmonic_zeta, d->harmonic_static ? "t" : "nil");
    if (d->harmonic_stress) fprintf(f, " :stress t");                          /* written only when set */
    fprintf(f, ")");
  }
  if (d->transient_steps > 0) {                                                /* written only when asked for */
    static const char *shape[] = {"step", "ramp", "half-sine"};
    fprintf(f, "\n   (transient :steps %d :dt %.17g :shape %s :rise %.17g :zeta %.17g :static-correction %s", d->transient_steps,
            d->transient_dt, shape[d->transient_shape], d->transient_rise, d->transient_zeta, d->transient_static ? "t" : "nil");
    if (d->transient_has_base)
      fprintf(f, " :base (%.17g %.17g %.17g)", d->transient_base[0], d->transient_base[1], d->transient_base[2]);
    if (d->transient_stress) fprintf(f, " :stress t");                         /* written only when set */
    if (d->transient_sn_exponent > 0)                                          /* written only when set */
      fprintf(f, " :sn-exponent %.17g :sn-coefficient %.17g :rainflow-depth %d", d->transient_sn_exponent, d->transient_sn_coefficient,
              d->transient_rainflow_depth);
    fprintf(f, ")");
  }
  if (d->has_spectrum) {                                                       /* written only when present */
    static const char *rule[] = {"srss", "cqc", "abs"};
    fprintf(f, "\n   (spectrum :rule %s :zeta %.17g :static-correction %s :zpa %.17g :interp %s", rule[d->spectrum_rule],
            d->spectrum_zeta, d->spectrum_static ? "t" : "nil", d->spectrum_zpa, d->spectrum_loglog ? "loglog" : "linear");
    if (d->spectrum_has_base)
      fprintf(f, " :base (%.17g %.17g %.17g)", d->spectrum_base[0], d->spectrum_base[1], d->spectrum_base[2]);
    if (d->spectrum_stress) fprintf(f, " :stress t");                          /* written only when set */
    fprintf(f, "\n    (points");
    for (i = 0; i < d->spectrum_count; ++i) fprintf(f, " (%.17g %.17g)", d->spectrum_points[2 * i], d->spectrum_points[2 * i + 1]);
    fprintf(f, "))");
  }
  if (d->has_random) {                                                         /* written only when present */
    fprintf(f, "\n   (random :zeta %.17g :static-correction %s :interp %s :per-mode %d :background %d", d->random_zeta,
            d->random_static ? "t" : "nil", d->random_loglog ? "loglog" : "linear", d->random_per_mode, d->random_background);
    if (d->random_has_base)
      fprintf(f, " :base (%.17g %.17g %.17g)", d->random_base[0], d->random_base[1], d->random_base[2]);
    if (d->random_stress) fprintf(f, " :stress t");
    if (d->random_sn_exponent > 0)                                             /* written only when set */
      fprintf(f, " :sn-exponent %.17g :sn-coefficient %.17g :duration %.17g", d->random_sn_exponent, d->random_sn_coefficient, d->random_duration);
    fprintf(f, "\n    (psd");
    for (i = 0; i < d->random_count; ++i) fprintf(f, " (%.17g %.17g)", d->random_points[2 * i], d->random_points[2 * i + 1]);
    fprintf(f, "))");
  }
  if (d->buckling_modes > 0)                                                   /* written only when asked for */
    fprintf(f, "\n   (buckling :modes %d :tolerance %.17g :max %d)", d->buckling_modes, d->buckling_tolerance, d->buckling_max);
  fprintf(f, ")\n");
  fprintf(f, " (input-data\n  (geometry\n   (nodes");
  for (i = 0; i < d->nodes_count; ++i)
    fprintf(f, "\n    (%.17g %.17g %.17g)", d->nodes[3 * i], d->nodes[3 * i + 1], d->nodes[3 * i + 2]);
  fprintf(f, ")\n   (elements");
  for (i = 0; i < d->elements_count; ++i) {
    fprintf(f, "\n    (");
    for (k = 0; k < d->nodes_per_element; ++k)
      fprintf(f, k ? " %d" : "%d", d->elements[(size_t)i * d->nodes_per_element + k]);
    fprintf(f, ")");
  }
  fprintf(f, ")");
  if (d->materials_count > 0) {
    fprintf(f, "\n   (element-materials");
    for (i = 0; i < d->elements_count; ++i) fprintf(f, i % 32 ? " %d" : "\n    %d", d->element_material[i]);
    fprintf(f, ")");
  }
  fprintf(f, ")\n  (boundary-conditions\n   (prescribed-displacements");
  for (i = 0; i < d->prescribed_nodes_count; ++i)
    fprintf(f, "\n    (presc-node :y %.17g :x %.17g :z %.17g :type %d :node-id %d)", d->presc_values[3 * i + 1],
            d->presc_values[3 * i], d->presc_values[3 * i + 2], d->presc_type[i], d->presc_node[i]);
  fprintf(f, ")");
  if (d->surface_faces_count > 0) {                  /* written only when there are faces: other decks save as before */
    fprintf(f, "\n   (surface-loads");
    for (i = 0; i < d->surface_faces_count; ++i) {
      const double *v = d->surface_values + 3 * (size_t)i;
      if (d->surface_kind[i] == FEAHIP_LOAD_PRESSURE) fprintf(f, "\n    (pressure :value %.17g :nodes (", v[0]);
      else fprintf(f, "\n    (traction :x %.17g :y %.17g :z %.17g :nodes (", v[0], v[1], v[2]);
      for (k = 0; k < d->surface_nodes_per_face; ++k)
        fprintf(f, k ? " %d" : "%d", d->surface_nodes[(size_t)i * d->surface_nodes_per_face + k]);
      fprintf(f, "))");
    }
    fprintf(f, ")");
  }
  if (d->contact_faces_count > 0 && d->contact_obstacles_count > 0) {   /* written only when there is contact */
    fprintf(f, "\n   (contact :penalty %.17g :augment %d :gap-tolerance %.17g\n    (faces", d->contact_penalty, d->contact_augment,
            d->contact_gap_tolerance);
    for (i = 0; i < d->contact_faces_count; ++i) {
      fprintf(f, "\n     (");
      for (k = 0; k < d->contact_nodes_per_face; ++k)
        fprintf(f, k ? " %d" : "%d", d->contact_nodes[(size_t)i * d->contact_nodes_per_face + k]);
      fprintf(f, ")");
    }
    fprintf(f, ")");
    for (i = 0; i < d->contact_obstacles_count; ++i) {
      const double *g = d->contact_geom + 10 * (size_t)i;
      const int kd = d->contact_kind[i];
      const int inside = kd == FEAHIP_OBSTACLE_SPHERE_INSIDE || kd == FEAHIP_OBSTACLE_CYLINDER_INSIDE;
      if (kd == FEAHIP_OBSTACLE_PLANE)
        fprintf(f, "\n    (plane :point (%.17g %.17g %.17g) :normal (%.17g %.17g %.17g)", g[0], g[1], g[2], g[3], g[4], g[5]);
      else if (kd == FEAHIP_OBSTACLE_SPHERE || kd == FEAHIP_OBSTACLE_SPHERE_INSIDE)
        fprintf(f, "\n    (sphere :center (%.17g %.17g %.17g) :radius %.17g", g[0], g[1], g[2], g[6]);
      else
        fprintf(f, "\n    (cylinder :point (%.17g %.17g %.17g) :axis (%.17g %.17g %.17g) :radius %.17g", g[0], g[1], g[2], g[3], g[4],
                g[5], g[6]);
      fprintf(f, " :travel (%.17g %.17g %.17g)", g[7], g[8], g[9]);
      if (kd != FEAHIP_OBSTACLE_PLANE) fprintf(f, " :inside %s", inside ? "t" : "nil");
      fprintf(f, ")");
    }
    fprintf(f, ")");
  }
  if (d->has_body_force)
    fprintf(f, "\n   (body-force :x %.17g :y %.17g :z %.17g)", d->body_force[0], d->body_force[1], d->body_force[2]);
  fprintf(f, ")))\n");
  return fclose(f);
}
