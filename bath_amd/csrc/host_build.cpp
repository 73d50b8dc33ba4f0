// host_build.cpp -- single-sequence models (bathbuild on an unaligned protein file): host code, no GPU.
//
//   bath_scoresystem_create   <- p7_builder_LoadScoreSystem / _SetScoreSystem    src/p7_builder.c:199-330
//   bath_hmm_from_sequence    <- p7_SingleBuilder up to calibrate()               src/p7_builder.c:501-532 (p7_Seqmodel, src/seqmodel.c:47-99;
//                                p7_hmm_SetComposition, p7_hmm_SetConsensus, src/p7_hmm.c:632, :709)
//   bath_hmm_mean_match_relent / bath_hmm_lambda <- p7_MeanMatchRelativeEntropy, p7_Lambda   src/modelstats.c:80, src/evalues.c:244
//   bath_hmm_write_ascii      <- p7_hmmfile_WriteASCII(fp, p7_BATH_3f, hmm)        src/p7_hmmfile.c:565-689
//
// easel is not part of the reference tree, so esl_scorematrix_Read (NCBI format), esl_scorematrix_ProbifyGivenBG (the root of
// sum_ab f_a f_b exp(lambda s_ab) = 1 by Newton-Raphson from the first doubling of 1 / max(s) at which the sum exceeds 1),
// esl_scorematrix_JointToConditionalOnQuery (each row over its sum), esl_vec_FRelEntropy and esl_vec_FNorm are restated from their
// published behaviour, as bath_calibrate.hip restates other easel pieces.  The floats of the model are the reference's: every
// narrowing (esl_vec_D2F of the matrix rows, the double gap arithmetic stored in float transitions) is where the reference has it.
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "bath_hip.h"
#include "host_model.hpp"

using namespace bath;

// BLOSUM62 in the NCBI text format esl_scorematrix_Read takes (the table of Henikoff & Henikoff 1992 as NCBI distributes it): the
// one built-in score system.  It goes through the same reader as an --mxfile file.
static const char kBlosum62[] =
    "#  Matrix made by matblas from blosum62.iij\n"
    "   A  R  N  D  C  Q  E  G  H  I  L  K  M  F  P  S  T  W  Y  V  B  Z  X  *\n"
    "A  4 -1 -2 -2  0 -1 -1  0 -2 -1 -1 -1 -1 -2 -1  1  0 -3 -2  0 -2 -1  0 -4\n"
    "R -1  5  0 -2 -3  1  0 -2  0 -3 -2  2 -1 -3 -2 -1 -1 -3 -2 -3 -1  0 -1 -4\n"
    "N -2  0  6  1 -3  0  0  0  1 -3 -3  0 -2 -3 -2  1  0 -4 -2 -3  3  0 -1 -4\n"
    "D -2 -2  1  6 -3  0  2 -1 -1 -3 -4 -1 -3 -3 -1  0 -1 -4 -3 -3  4  1 -1 -4\n"
    "C  0 -3 -3 -3  9 -3 -4 -3 -3 -1 -1 -3 -1 -2 -3 -1 -1 -2 -2 -1 -3 -3 -2 -4\n"
    "Q -1  1  0  0 -3  5  2 -2  0 -3 -2  1  0 -3 -1  0 -1 -2 -1 -2  0  3 -1 -4\n"
    "E -1  0  0  2 -4  2  5 -2  0 -3 -3  1 -2 -3 -1  0 -1 -3 -2 -2  1  4 -1 -4\n"
    "G  0 -2  0 -1 -3 -2 -2  6 -2 -4 -4 -2 -3 -3 -2  0 -2 -2 -3 -3 -1 -2 -1 -4\n"
    "H -2  0  1 -1 -3  0  0 -2  8 -3 -3 -1 -2 -1 -2 -1 -2 -2  2 -3  0  0 -1 -4\n"
    "I -1 -3 -3 -3 -1 -3 -3 -4 -3  4  2 -3  1  0 -3 -2 -1 -3 -1  3 -3 -3 -1 -4\n"
    "L -1 -2 -3 -4 -1 -2 -3 -4 -3  2  4 -2  2  0 -3 -2 -1 -2 -1  1 -4 -3 -1 -4\n"
    "K -1  2  0 -1 -3  1  1 -2 -1 -3 -2  5 -1 -3 -1  0 -1 -3 -2 -2  0  1 -1 -4\n"
    "M -1 -1 -2 -3 -1  0 -2 -3 -2  1  2 -1  5  0 -2 -1 -1 -1 -1  1 -3 -1 -1 -4\n"
    "F -2 -3 -3 -3 -2 -3 -3 -3 -1  0  0 -3  0  6 -4 -2 -2  1  3 -1 -3 -3 -1 -4\n"
    "P -1 -2 -2 -1 -3 -1 -1 -2 -2 -3 -3 -1 -2 -4  7 -1 -1 -4 -3 -2 -2 -1 -2 -4\n"
    "S  1 -1  1  0 -1  0  0  0 -1 -2 -2  0 -1 -2 -1  4  1 -3 -2 -2  0  0  0 -4\n"
    "T  0 -1  0 -1 -1 -1 -1 -2 -2 -1 -1 -1 -1 -2 -1  1  5 -2 -2  0 -1 -1  0 -4\n"
    "W -3 -3 -4 -4 -2 -2 -3 -2 -2 -3 -2 -3 -1  1 -4 -3 -2 11  2 -3 -4 -3 -2 -4\n"
    "Y -2 -2 -2 -3 -2 -1 -2 -3  2 -1 -1 -2 -1  3 -3 -2 -2  2  7 -1 -3 -2 -1 -4\n"
    "V  0 -3 -3 -3 -1 -2 -2 -3 -3  3  1 -2  1 -1 -2 -2  0 -3 -1  4 -3 -2 -1 -4\n"
    "B -2 -1  3  4 -3  0  1 -1  0 -3 -4  0 -3 -3 -2  0 -1 -4 -3 -3  4  1 -1 -4\n"
    "Z -1  0  0  1 -3  3  4 -2  0 -3 -3  1 -1 -3 -1  0 -1 -3 -2 -2  1  4 -1 -4\n"
    "X  0 -1 -1 -1 -2 -1 -1 -1 -1 -1 -1 -1 -1 -1 -2  0  0 -2 -1 -1 -1 -1 -1 -4\n"
    "* -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4  1\n";

static const char kAminoK[] = "ACDEFGHIKLMNPQRSTVWY";

struct bath_scoresystem {
  int    s[20][20];         // scores of the 20 residues, easel order
  double Q[20][20];         // P(b | a): row a is the match emission vector of a query residue a
  double lambda, popen, pextend;
};

static void set_err(char *errbuf, int errlen, const std::string &msg) {
  if (errbuf && errlen > 0) std::snprintf(errbuf, (size_t)errlen, "%s", msg.c_str());
}

// esl_scorematrix_Read: '#' comments and blank lines skipped; a header line of residue symbols; then one row per symbol, its own
// symbol first (optional in the format; required here), in the header's order.  Symbols outside the 20 residues (B Z X * J O U) are
// read and dropped: a single-sequence model indexes the 20 x 20 core only.  Every one of the 20 residues must be there.
static int read_ncbi_matrix(std::istream &in, int s[20][20], std::string *why) {
  std::string line;
  std::vector<int> col;                 // header position -> residue code, -1: a symbol outside the 20
  bool seen[20] = {false};
  int nrow = 0;
  while (std::getline(in, line)) {
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.erase(hash);
    std::istringstream ss(line);
    std::vector<std::string> tk;
    for (std::string t; ss >> t;) tk.push_back(t);
    if (tk.empty()) continue;
    if (col.empty()) {
      for (const std::string &t : tk) {
        if (t.size() != 1) { *why = "the header line holds " + t + ", not a single residue symbol"; return BATH_EFORMAT; }
        const char *p = std::strchr(kAminoK, std::toupper((unsigned char)t[0]));
        col.push_back(p && *p ? (int)(p - kAminoK) : -1);
      }
      continue;
    }
    if ((size_t)nrow >= col.size()) { *why = "more rows than the header has symbols"; return BATH_EFORMAT; }
    if (tk.size() != col.size() + 1 || tk[0].size() != 1) { *why = "row " + std::to_string(nrow + 1) + " does not hold its symbol and " + std::to_string(col.size()) + " scores"; return BATH_EFORMAT; }
    const char *p = std::strchr(kAminoK, std::toupper((unsigned char)tk[0][0]));
    const int a = p && *p ? (int)(p - kAminoK) : -1;
    if (a != col[(size_t)nrow]) { *why = "row " + std::to_string(nrow + 1) + " is labelled " + tk[0] + ", out of the header's order"; return BATH_EFORMAT; }
    if (a >= 0) {
      for (size_t j = 0; j < col.size(); j++) {
        char *end = nullptr;
        const long v = std::strtol(tk[j + 1].c_str(), &end, 10);
        if (!end || *end) { *why = "row " + std::to_string(nrow + 1) + " holds " + tk[j + 1] + ", not an integer score"; return BATH_EFORMAT; }
        if (col[j] >= 0) s[a][col[j]] = (int)v;
      }
      seen[a] = true;
    }
    nrow++;
  }
  if (col.empty()) { *why = "no header line of residue symbols"; return BATH_EFORMAT; }
  for (int a = 0; a < 20; a++)
    if (!seen[a]) { *why = std::string("no row for residue ") + kAminoK[a]; return BATH_EFORMAT; }
  for (int a = 0; a < 20; a++) {
    bool in_header = false;
    for (int c : col) in_header |= (c == a);
    if (!in_header) { *why = std::string("no column for residue ") + kAminoK[a]; return BATH_EFORMAT; }
  }
  return BATH_OK;
}

// lambda_fdf of esl_scorematrix.c: f = sum_ab f_a f_b exp(lambda s_ab) - 1 and its derivative
static void lambda_fdf(const int s[20][20], const double *f, double lambda, double *fx, double *dfx) {
  *fx = 0.; *dfx = 0.;
  for (int i = 0; i < 20; i++)
    for (int j = 0; j < 20; j++) {
      const double e = f[i] * f[j] * std::exp(lambda * (double)s[i][j]);
      *fx += e;
      *dfx += e * (double)s[i][j];
    }
  *fx -= 1.0;
}

// esl_scorematrix_ProbifyGivenBG with fi = fj = f.  BATH_EINVAL: no positive root (the sum never exceeds 1 below lambda = 50);
// BATH_ENORESULT: Newton-Raphson did not halt.
static int solve_lambda(const int s[20][20], const double *f, double *ret_lambda) {
  int smax = s[0][0];
  for (int i = 0; i < 20; i++) for (int j = 0; j < 20; j++) smax = std::max(smax, s[i][j]);
  if (smax <= 0) return BATH_EINVAL;
  double fx = 0., dfx = 0., x = 1. / (double)smax;
  for (; x < 50.; x *= 2.0) { lambda_fdf(s, f, x, &fx, &dfx); if (fx > 0) break; }
  if (!(fx > 0)) return BATH_EINVAL;
  for (int iter = 0; iter < 100; iter++) {                    // esl_root_NewtonRaphson at its default tolerances (relative 1e-15)
    const double x0 = x;
    x = x - fx / dfx;
    lambda_fdf(s, f, x, &fx, &dfx);
    if (fx == 0. || std::fabs(x - x0) < 1e-15 * x) { *ret_lambda = x; return BATH_OK; }
  }
  return BATH_ENORESULT;
}

extern "C" const char *bath_scorematrix_builtin(const char *name) {
  return name && std::strcmp(name, "BLOSUM62") == 0 ? kBlosum62 : nullptr;
}

extern "C" int bath_scoresystem_create(const char *mx_name, const char *mxfile, double popen, double pextend, bath_scoresystem **ret,
                                       char *errbuf, int errlen) {
  if (!ret) return BATH_EINVAL;
  *ret = nullptr;
  if (!(popen >= 0. && popen < 0.5) || !(pextend >= 0. && pextend < 1.)) { set_err(errbuf, errlen, "gap probabilities need 0 <= popen < 0.5 and 0 <= pextend < 1"); return BATH_EINVAL; }
  bath_scoresystem *S = new bath_scoresystem();
  std::memset(S, 0, sizeof *S);
  std::string why, what;
  int st;
  if (mxfile) {
    what = mxfile;
    std::ifstream in(mxfile);
    if (!in) { delete S; set_err(errbuf, errlen, std::string("score matrix file ") + mxfile + " not found or not readable"); return BATH_EFAIL; }
    st = read_ncbi_matrix(in, S->s, &why);
    if (st != BATH_OK) { delete S; set_err(errbuf, errlen, std::string("error parsing score matrix file ") + mxfile + ":\n" + why); return st; }
  } else {
    what = mx_name ? mx_name : "BLOSUM62";
    const char *text = bath_scorematrix_builtin(what.c_str());
    if (!text) { delete S; set_err(errbuf, errlen, "no matrix named " + what + " is available as a built-in"); return BATH_EFAIL; }   // p7_builder.c:214
    std::istringstream in(text);
    st = read_ncbi_matrix(in, S->s, &why);
    if (st != BATH_OK) { delete S; set_err(errbuf, errlen, "failed to set score matrix " + what + " as a built-in"); return st; }
  }
  double f[20];
  for (int a = 0; a < 20; a++) f[a] = (double)kAminoBg[a];                   // esl_vec_F2D(bg->f)
  st = solve_lambda(S->s, f, &S->lambda);
  if (st != BATH_OK) {                                                        // p7_builder.c:224-225, :310-311
    const std::string kind = mxfile ? "input score matrix " : "built-in score matrix ";
    set_err(errbuf, errlen, st == BATH_EINVAL ? kind + what + " has no valid solution for lambda" : "failed to solve score matrix " + what + " for lambda");
    delete S;
    return BATH_EINVAL;
  }
  for (int a = 0; a < 20; a++) {
    double row = 0.;
    for (int b = 0; b < 20; b++) { S->Q[a][b] = f[a] * f[b] * std::exp(S->lambda * (double)S->s[a][b]); row += S->Q[a][b]; }   // P(a, X): the row's sum
    for (int b = 0; b < 20; b++) S->Q[a][b] = row == 0.0 ? 0.0 : S->Q[a][b] / row;
  }
  S->popen = popen; S->pextend = pextend;
  *ret = S;
  return BATH_OK;
}

extern "C" void bath_scoresystem_destroy(bath_scoresystem *s) { delete s; }
extern "C" double bath_scoresystem_lambda(const bath_scoresystem *s) { return s ? s->lambda : 0.; }
extern "C" int bath_scoresystem_conditionals(const bath_scoresystem *s, double *Q) {
  if (!s || !Q) return BATH_EINVAL;
  std::memcpy(Q, s->Q, sizeof s->Q);
  return BATH_OK;
}

// p7_hmm_CalculateOccupancy with the insert occupancies (p7_hmm.c:1348)
static void occupancy(const bath_hmm &h, std::vector<float> &mocc, std::vector<float> &iocc) {
  enum { MM = 0, MI, MD, IM, II, DM, DD };
  auto t = [&](int k, int x) { return h.t[(size_t)k * 7 + x]; };
  mocc[0] = 0.f;
  mocc[1] = t(0, MI) + t(0, MM);
  for (int k = 2; k <= h.M; k++) mocc[(size_t)k] = (float)(mocc[(size_t)k - 1] * (t(k - 1, MM) + t(k - 1, MI)) + (1.0 - mocc[(size_t)k - 1]) * t(k - 1, DM));
  iocc[0] = t(0, MI) / t(0, IM);
  for (int k = 1; k <= h.M; k++) iocc[(size_t)k] = mocc[(size_t)k] * t(k, MI) / t(k, IM);
}

extern "C" int bath_hmm_from_sequence(const bath_scoresystem *S, const uint8_t *dsq, int n, const char *name, int ct, bath_hmm **ret) {
  if (!ret) return BATH_EINVAL;
  *ret = nullptr;
  if (!S || !dsq || n < 1 || !name) return BATH_EINVAL;
  if (std::strlen(name) >= sizeof(((bath_hmm *)nullptr)->name)) return BATH_ERANGE;   // a name bath_hmm cannot hold whole is refused, not cut
  for (int i = 0; i < n; i++) if (dsq[i] >= 20) return BATH_EINVAL;          // residues only: the caller strips and refuses first
  uint8_t basic[64];
  if (bath_gencode_basic(ct, basic) != BATH_OK) return BATH_EINVAL;
  const int M = n;
  bath_hmm *h = new bath_hmm();
  std::memset(h, 0, sizeof *h);
  h->M = M; h->max_length = -1; h->ct = ct; h->fsprob = 0.01f;              // p7P_FSPROB
  for (float &e : h->evparam) e = -99999.0f;                                 // p7_EVPARAM_UNSET
  std::snprintf(h->name, sizeof h->name, "%s", name);
  h->t = new float[(size_t)(M + 1) * 7]();
  h->mat = new float[(size_t)(M + 1) * 20]();
  h->ins = new float[(size_t)(M + 1) * 20]();
  h->consensus = new char[(size_t)M + 2]();
  const double popen = S->popen, pextend = S->pextend;
  for (int k = 0; k <= M; k++) {                                             // seqmodel.c:59-74
    if (k > 0) for (int x = 0; x < 20; x++) h->mat[(size_t)k * 20 + x] = (float)S->Q[dsq[k - 1]][x];
    for (int x = 0; x < 20; x++) h->ins[(size_t)k * 20 + x] = kAminoBg[x];
    float *t = h->t + (size_t)k * 7;
    t[0] = (float)(1.0 - 2 * popen); t[1] = (float)popen; t[2] = (float)popen;
    t[3] = (float)(1.0 - pextend);   t[4] = (float)pextend;
    t[5] = (float)(1.0 - pextend);   t[6] = (float)pextend;
  }
  float *tM = h->t + (size_t)M * 7;                                          // seqmodel.c:79-82
  tM[0] = (float)(1.0 - popen); tM[2] = 0.f; tM[5] = 1.0f; tM[6] = 0.f;

  std::vector<float> mocc((size_t)M + 1), iocc((size_t)M + 1);               // p7_hmm_SetComposition
  occupancy(*h, mocc, iocc);
  for (int x = 0; x < 20; x++) h->compo[x] = 0.f;
  for (int x = 0; x < 20; x++) h->compo[x] += h->ins[x] * iocc[0];
  for (int k = 1; k <= M; k++) {
    for (int x = 0; x < 20; x++) h->compo[x] += h->mat[(size_t)k * 20 + x] * mocc[(size_t)k];
    for (int x = 0; x < 20; x++) h->compo[x] += h->ins[(size_t)k * 20 + x] * iocc[(size_t)k];
  }
  float sum = 0.f, comp = 0.f;                                               // esl_vec_FNorm: compensated sum, then divide
  for (int x = 0; x < 20; x++) { const float y = h->compo[x] - comp, t = sum + y; comp = (t - sum) - y; sum = t; }
  for (int x = 0; x < 20; x++) h->compo[x] = sum != 0.f ? h->compo[x] / sum : 1.f / 20.f;

  h->consensus[0] = ' ';                                                     // p7_hmm_SetConsensus(hmm, sq): the sequence itself
  for (int k = 1; k <= M; k++) {
    const int x = dsq[k - 1];
    h->consensus[k] = h->mat[(size_t)k * 20 + x] >= 0.5f ? kAminoK[x] : (char)std::tolower(kAminoK[x]);
  }
  *ret = h;
  return BATH_OK;
}

extern "C" double bath_hmm_mean_match_relent(const bath_hmm *hmm) {
  if (!hmm || hmm->M < 1) return 0.;
  double KL = 0.;
  for (int k = 1; k <= hmm->M; k++) {                                        // esl_vec_FRelEntropy: a float sum, scaled to bits
    const float *p = hmm->mat + (size_t)k * 20;
    float kl = 0.f;
    for (int x = 0; x < 20; x++)
      if (p[x] > 0.f) kl = (float)(kl + p[x] * std::log((double)(p[x] / kAminoBg[x])));
    KL += (double)(float)(1.44269504 * kl);
  }
  return KL / (double)hmm->M;
}

static float fsum(const float *v, int n) {                                    // esl_vec_FSum: a compensated float sum
  float sum = 0.f, c = 0.f;
  for (int i = 0; i < n; i++) { const float y = v[i] - c, t = sum + y; c = (t - sum) - y; sum = t; }
  return sum;
}

// p7_MeanPositionRelativeEntropy (modelstats.c:163): the match emissions' relative entropy weighted by match occupancy
// (p7_hmm_CalculateOccupancy, p7_hmm.c:1348), plus the occupancy-weighted cost in bits of the transitions into nodes 2..M against
// the background's p1 = 350/351.  bathstat's last column; not the unweighted figure above that bathbuild prints.
extern "C" double bath_hmm_mean_position_relent(const bath_hmm *hmm) {
  if (!hmm || hmm->M < 1) return 0.;
  const int M = hmm->M;
  const float p1 = 350.f / 351.f;                                            // p7_bg_Create
  const float *t = hmm->t;                                                   // [k][MM MI MD IM II DM DD]
  std::vector<float> mocc((size_t)M + 1);
  mocc[0] = 0.f;
  mocc[1] = t[1] + t[0];
  for (int k = 2; k <= M; k++) {
    const float *tk = t + (size_t)(k - 1) * 7;
    mocc[(size_t)k] = (float)(mocc[(size_t)k - 1] * (tk[0] + tk[1]) + (1.0 - mocc[(size_t)k - 1]) * tk[5]);
  }
  double mre = 0., tre = 0.;
  for (int k = 1; k <= M; k++) {                                             // esl_vec_FRelEntropy, as above
    const float *p = hmm->mat + (size_t)k * 20;
    float kl = 0.f;
    for (int x = 0; x < 20; x++)
      if (p[x] > 0.f) kl = (float)(kl + p[x] * std::log((double)(p[x] / kAminoBg[x])));
    mre += mocc[(size_t)k] * (float)(1.44269504 * kl);
  }
  mre /= fsum(mocc.data() + 1, M);
  for (int k = 2; k <= M; k++) {
    const float *tk = t + (size_t)(k - 1) * 7;
    const float m1 = mocc[(size_t)k - 1];
    const double xm = m1 * tk[0] * std::log((double)(tk[0] / p1));
    const double xi = m1 * tk[1] * (std::log((double)(tk[0] / p1)) + std::log((double)(tk[3] / p1)));
    const double xd = (1. - m1) * tk[5] * std::log((double)(tk[5] / p1));
    tre += (xm + xi + xd) / 0.69314718055994529;
  }
  tre /= fsum(mocc.data() + 2, M - 1);                                       // (M = 1: 0 / 0, as the reference has it)
  return mre + tre;
}

extern "C" double bath_hmm_lambda(const bath_hmm *hmm) {
  if (!hmm || hmm->M < 1) return 0.;
  return 0.69314718055994529 + 1.44 / ((double)hmm->M * bath_hmm_mean_match_relent(hmm));
}

static void printprob(std::string &out, float p) {                            // p7_hmmfile.c:2201
  char b[32];
  if (p == 0.0f) std::snprintf(b, sizeof b, " %*s", 8, "*");
  else if (p == 1.0f) std::snprintf(b, sizeof b, " %*.5f", 8, 0.0);
  else std::snprintf(b, sizeof b, " %*.5f", 8, (double)-logf(p));
  out += b;
}

extern "C" int64_t bath_hmm_write_ascii(const bath_hmm *hmm, int nseq, double eff_nseq, const char *desc, const char *date, const char *comlog,
                                        char *buf, int64_t cap) {
  if (!hmm || hmm->M < 1 || !hmm->t || !hmm->mat || !hmm->ins) return -1;
  std::string o;
  char b[256];
  auto line = [&](const char *fmt, auto... a) { std::snprintf(b, sizeof b, fmt, a...); o += b; };
  o += "BATH3/f\n";
  line("NAME  %s\n", hmm->name);
  if (hmm->acc[0]) line("ACC   %s\n", hmm->acc);
  if (desc && desc[0]) { o += "DESC  "; o += desc; o += "\n"; }
  line("LENG  %d\n", hmm->M);
  if (hmm->max_length > 0) line("MAXL  %d\n", hmm->max_length);
  o += "ALPH  amino\n";
  line("RF    %s\n", hmm->rf ? "yes" : "no");
  o += "MM    no\n";
  line("CONS  %s\n", hmm->consensus ? "yes" : "no");
  line("CS    %s\n", hmm->cs ? "yes" : "no");
  o += "MAP   no\n";
  if (date && date[0]) { o += "DATE  "; o += date; o += "\n"; }
  if (comlog && comlog[0]) {                                                  // multiline(fp, "COM  ", comlog): one numbered line per command
    std::istringstream ss(comlog);
    int n = 1;
    for (std::string ln; std::getline(ss, ln); n++) { line("COM   [%d] ", n); o += ln; o += "\n"; }
  }
  if (nseq > 0) line("NSEQ  %d\n", nseq);
  if (eff_nseq >= 0) line("EFFN  %f\n", (double)(float)eff_nseq);
  if (hmm->evparam[0] != -99999.0f) {                                         // p7H_STATS
    const float *e = hmm->evparam;
    line("STATS LOCAL MSV         %8.4f %8.5f\n", (double)e[0], (double)e[1]);
    line("STATS LOCAL VITERBI     %8.4f %8.5f\n", (double)e[2], (double)e[3]);
    line("STATS LOCAL FORWARD     %8.4f %8.5f\n", (double)e[4], (double)e[5]);
    if (e[6] != -99999.0f && e[7] != -99999.0f) {                             // hmm->fs (p7_hmmfile.c:620-622): the taus were fitted
      line("STATS LOCAL FS3 FORWARD %8.4f %8.5f\n", (double)e[6], (double)e[5]);
      line("STATS LOCAL FS5 FORWARD %8.4f %8.5f\n", (double)e[7], (double)e[5]);
      line("FRAMESHIFT PROB  %8.4f\n", (double)hmm->fsprob);
    }
    if (hmm->ct) line("CODON TABLE  %d\n", hmm->ct);
  }
  o += "HMM     ";
  for (int x = 0; x < 20; x++) line("     %c   ", kAminoK[x]);
  o += "\n";
  line("        %8s %8s %8s %8s %8s %8s %8s\n", "m->m", "m->i", "m->d", "i->m", "i->i", "d->m", "d->d");
  bool has_compo = false;
  for (int x = 0; x < 20; x++) has_compo |= hmm->compo[x] != 0.f;
  if (has_compo) {
    o += "  COMPO ";
    for (int x = 0; x < 20; x++) printprob(o, hmm->compo[x]);
    o += "\n";
  }
  o += "        ";
  for (int x = 0; x < 20; x++) printprob(o, hmm->ins[x]);
  o += "\n        ";
  for (int x = 0; x < 7; x++) printprob(o, hmm->t[x]);
  o += "\n";
  for (int k = 1; k <= hmm->M; k++) {
    line(" %6d ", k);
    for (int x = 0; x < 20; x++) printprob(o, hmm->mat[(size_t)k * 20 + x]);
    line(" %6s", "-");
    line(" %c", hmm->consensus ? hmm->consensus[k] : '-');
    line(" %c", hmm->rf ? hmm->rf[k] : '-');
    o += " -";
    line(" %c\n", hmm->cs ? hmm->cs[k] : '-');
    o += "        ";
    for (int x = 0; x < 20; x++) printprob(o, hmm->ins[(size_t)k * 20 + x]);
    o += "\n        ";
    for (int x = 0; x < 7; x++) printprob(o, hmm->t[(size_t)k * 7 + x]);
    o += "\n";
  }
  o += "//\n";
  if (buf && cap > 0) std::memcpy(buf, o.data(), (size_t)std::min<int64_t>(cap, (int64_t)o.size()));
  return (int64_t)o.size();
}
