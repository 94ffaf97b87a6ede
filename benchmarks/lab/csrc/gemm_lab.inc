// Lab build only (-DDVD_LAB), included by dvd_amd/csrc/gemm.hip after gemm_select: every DVD_GEMM_* switch, the experiment
// instances of the GEMM family and dvd_gemm_debug_stamps.  The switches are read here, on every call, and nowhere else.

static unsigned long long* g_gemm_stamps = nullptr;
// DVD_GEMM_DEBUG=3 / DVD_GEMM_T384_DBG=5: where the per-wave s_memtime stamps of the large-tile kernels go
extern "C" int dvd_gemm_debug_stamps(void* dev_u64) { g_gemm_stamps = (unsigned long long*)dev_u64; return DVD_OK; }

namespace {
enum { LAB_RING, LAB_BIG16, LAB_BIG2, LAB_W8, LAB_PD4 /* + f32 */, LAB_BIG = 6 /* + variant - 1 */ };
const GemmKernel kGemmLab[] = {
    // the split kernel's 3-stage skewed pipeline on one weight tensor, for A/B runs against gemm_nt_big_kernel
    GEMM_INSTANCE(512, 3 * 3 * 256 * 64, 256, 256, true, "gemm_nt(ring, lab)", gemm_nt_split_kernel<false>),
    // the 16x16x32-MFMA variant of the 256 x 256 kernel (measured 1-7 % slower, see gemm_nt_big16_kernel)
    GEMM_INSTANCE(512, 2 * 2 * 256 * 128, 256, 256, true, "gemm_nt(big16)", gemm_nt_big16_kernel),
    GEMM_INSTANCE(256, big2::NBUF * big2::HALF, 256, 256, true, "gemm_nt(big2)", gemm_nt_big2_kernel),
    // two waves per SIMD on each 128 x 128 tile
    GEMM_INSTANCE(512, 0, 128, 128, false, "gemm_nt(w8, lab)", gemm_nt_w8_kernel),
    // register prefetch four tiles deep (measured: no gain, see gemm_nt_kernel)
    GEMM_INSTANCE(256, 0, 128, 128, false, "gemm_nt(pd4, lab)", gemm_nt_kernel<false, 4, false>),
    GEMM_INSTANCE(256, 0, 128, 128, false, "gemm_nt(pd4, lab)", gemm_nt_kernel<true, 4, false>),
    // gemm_nt_big_kernel's timing ablations (DVD_GEMM_DEBUG) and <4>, the spread start (DVD_GEMM_SPREAD)
    GEMM_INSTANCE(512, 2 * 2 * 256 * 128, 256, 256, true, "gemm_nt(big)", gemm_nt_big_kernel<1>),
    GEMM_INSTANCE(512, 2 * 2 * 256 * 128, 256, 256, true, "gemm_nt(big)", gemm_nt_big_kernel<2>),
    GEMM_INSTANCE(512, 2 * 2 * 256 * 128, 256, 256, true, "gemm_nt(big)", gemm_nt_big_kernel<3>),
    GEMM_INSTANCE(512, 2 * 2 * 256 * 128, 256, 256, true, "gemm_nt(big)", gemm_nt_big_kernel<4>),
    GEMM_INSTANCE(512, 2 * 2 * 256 * 128, 256, 256, true, "gemm_nt(big)", gemm_nt_big_kernel<5>),
    GEMM_INSTANCE(512, 2 * 2 * 256 * 128, 256, 256, true, "gemm_nt(big)", gemm_nt_big_kernel<6>),
    GEMM_INSTANCE(512, 2 * 2 * 256 * 128, 256, 256, true, "gemm_nt(big)", gemm_nt_big_kernel<7>),
};

// Every switch: the knobs of gemm_select, then what gemm_choose and gemm_tweak apply themselves.
struct GemmLab : GemmKnobs {
  bool ring = false, m16 = false, big2 = false, w8 = false, pd4 = false, spread = false, nonpersistent = false;
  int stagger = 0;                                           // measured: no effect
  int t384_stagger = T384_STAGGER, t384_walk = T384_WALK;
  int t384_debug = 0;                                        // GemmArgs::debug bits 0x100 .. 0x800
  int t384_nblk = 256;                                       // fewer persistent workgroups
};

GemmLab gemm_lab_switches() {
  GemmLab s;
  auto num = [](const char* name, int otherwise) { const char* e = getenv(name); return e ? atoi(e) : otherwise; };
  s.scalar_epilogue = getenv("DVD_GEMM_SCALAR_EPILOGUE");
  s.v1 = getenv("DVD_GEMM_V1");
  s.twopass = getenv("DVD_GEMM_TWOPASS");
  s.debug = num("DVD_GEMM_DEBUG", 0);
  s.no_t384 = getenv("DVD_GEMM_NO_T384") || s.debug;
  s.ring128 = num("DVD_GEMM_RING128", 1) != 0;
  s.ring256 = num("DVD_GEMM_RING256", 1);
  // the t384 instance: with the 16x16x32 loop only the stamp build (5), with the 32x32x16 loop the ablations 1..6
  const int tdbg = num("DVD_GEMM_T384_DBG", 0);
  s.t384_x16 = getenv("DVD_GEMM_T384_M32") ? false : (getenv("DVD_GEMM_T384_X16") ? true : (T384_X16 != 0));
  s.t384_dbg = s.t384_x16 ? (tdbg == 5 ? 5 : 0) : (tdbg >= 1 && tdbg <= 6 ? tdbg : 0);
  s.ring = getenv("DVD_GEMM_RING");
  s.m16 = getenv("DVD_GEMM_M16");
  s.big2 = getenv("DVD_GEMM_BIG2");
  s.w8 = num("DVD_GEMM_W8", 0) != 0;
  s.pd4 = getenv("DVD_GEMM_PD4");
  s.spread = getenv("DVD_GEMM_SPREAD");
  s.nonpersistent = getenv("DVD_GEMM_NONPERSISTENT");
  s.stagger = num("DVD_GEMM_STAGGER", 0);
  s.t384_stagger = num("DVD_GEMM_T384_STAGGER", T384_STAGGER);
  s.t384_walk = num("DVD_GEMM_T384_WALK", T384_WALK);
  s.t384_debug = (getenv("DVD_GEMM_T384_PRIO") ? 0x100 : 0) | (getenv("DVD_GEMM_T384_NT") ? 0x200 : 0) |
                 (getenv("DVD_GEMM_T384_RES_PHASED") ? 0x400 : 0) | (getenv("DVD_GEMM_T384_NOSTORE") ? 0x800 : 0);
  s.t384_nblk = num("DVD_GEMM_T384_NBLK", 256);
  return s;
}

bool is_t384(const GemmKernel* k) { return k->tile_m == 384; }
bool is_big(const GemmKernel* k) { return k == &kGemm[BIG] || (k >= &kGemmLab[LAB_BIG] && k < &kGemmLab[LAB_BIG + 7]); }
}  // namespace

// gemm_select under the switches, then the experiment instances in place of the product's choice.
static int gemm_choose(const dvd_gemm_desc* d, GemmChoice& c) {
  const GemmLab s = gemm_lab_switches();
  if (const int rc = gemm_select(d, s, c); rc != DVD_OK) return rc;
  if ((is_t384(c.k) || c.k == &kGemm[BIG]) && !d->B_lo && !d->A_lo) {
    // the unsplit large-tile problems (what gemm_select gives gemm_nt_t384_kernel or gemm_nt_big_kernel)
    const bool plain_epilogue = c.vec_epilogue && !d->pos && !d->gate;
    const GemmKernel* k = nullptr;
    if (s.ring && d->K % 32 == 0) k = &kGemmLab[LAB_RING];
    else if (s.m16 && plain_epilogue) k = &kGemmLab[LAB_BIG16];
    else if (s.big2 && d->K % 32 == 0 && plain_epilogue && !(d->bias && d->bias_row)) k = &kGemmLab[LAB_BIG2];
    if (k) {
      c.k = k;
      c.stagger = c.walk = 0;
    }
  }
  if (c.k == &kGemm[BIG]) {
    const int dv = s.debug;
    const int variant = (dv == 1 || dv == 2 || dv == 3 || dv == 5 || dv == 6 || dv == 7) ? dv : s.spread ? 4 : 0;
    if (variant) c.k = &kGemmLab[LAB_BIG + variant - 1];
  }
  if (c.k == &kGemm[PLAIN] || c.k == &kGemm[PLAIN + 1]) {   // everything else declined
    if (s.w8 && d->dtype != 1) c.k = &kGemmLab[LAB_W8];
    else if (s.pd4) c.k = &kGemmLab[LAB_PD4 + (d->dtype == 1 ? 1 : 0)];
  }
  return DVD_OK;
}

// The argument and grid switches, just before the launch.
static void gemm_tweak(const GemmChoice& c, GemmArgs& p, int& max_wg) {
  const GemmLab s = gemm_lab_switches();
  p.stamps = g_gemm_stamps;
  p.stagger = s.stagger;
  if (is_t384(c.k)) {
    p.stagger = s.t384_stagger;
    p.walk = s.t384_walk;
    p.debug |= s.t384_debug;
    if (s.t384_nblk < max_wg) max_wg = s.t384_nblk;
  }
  if (s.nonpersistent && is_big(c.k)) max_wg = 1 << 30;
}
