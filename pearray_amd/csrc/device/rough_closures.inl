// rough_closures.inl -- the rough / principled closures' entry points, which fetch their own material spectra.  render.hip includes this file
// TWICE: with PR_CLOSURES_IMG 0 it defines spectrum_eval_cold, principled_closure, rough_eval and rough_sample as every variant without
// FEAT_IMAGES calls them; with PR_CLOSURES_IMG 1 their _uv forms, which take the shading point's uv and look image textures up there
// (the FEAT_IMAGES variants).  One text, two compilations: the plain forms stay, token for token, what they were before image textures
// (a shared body behind two wrappers reordered the operands of their products -- tools/code_identity.py holds the lower variants to their code).
#if PR_CLOSURES_IMG
#define PR_UV(name) name##_uv
#define PR_UV_PARAM , const float* uv
#define PR_UV_ARG , uv
#else
#define PR_UV(name) name
#define PR_UV_PARAM
#define PR_UV_ARG
#endif
// (FEAT_EXPR rides with FEAT_IMAGES, render.h: the _uv forms are also the ones that run an expression root's program)
static __device__ PR_CLOSURE Blob PR_UV(spectrum_eval_cold)(const DevScene& sc, uint32_t id, const Blob& wl PR_UV_PARAM) { return spectrum_eval<PR_CLOSURES_IMG != 0, PR_CLOSURES_IMG != 0>(sc, id, wl PR_UV_ARG); }
__device__ __forceinline__ Principled PR_UV(principled_closure)(const DevScene& s, const prgpu_material& m, const Blob& wl, const Blob& cie_y PR_UV_PARAM) // createClosure :475-497, ctor :63-84
{
	Principled p;
	p.base = PR_UV(spectrum_eval_cold)(s, m.albedo, wl PR_UV_ARG);
	p.ior  = PR_UV(spectrum_eval_cold)(s, m.ior, wl PR_UV_ARG);
	p.cie_y = cie_y;
	p.has_trans		  = (m.flags & PRGPU_MATF_HAS_TRANSMISSION) != 0;
	p.thin			  = m.thin != 0;
	p.vndf			  = (m.flags & PRGPU_MATF_NO_VNDF) == 0;
	p.diff_trans	  = p.has_trans ? m.principled[PRGPU_PRINCIPLED_DIFFUSE_TRANSMISSION] : 0.0f;
	p.spec_trans	  = p.has_trans ? m.principled[PRGPU_PRINCIPLED_SPECULAR_TRANSMISSION] : 0.0f;
	p.roughness		  = m.roughness_x;
	p.anisotropic	  = m.principled[PRGPU_PRINCIPLED_ANISOTROPIC];
	p.spec_tint		  = m.principled[PRGPU_PRINCIPLED_SPECULAR_TINT];
	p.flatness		  = m.principled[PRGPU_PRINCIPLED_FLATNESS];
	p.metallic		  = m.principled[PRGPU_PRINCIPLED_METALLIC];
	p.sheen			  = m.principled[PRGPU_PRINCIPLED_SHEEN];
	p.sheen_tint	  = m.principled[PRGPU_PRINCIPLED_SHEEN_TINT];
	p.clearcoat		  = m.principled[PRGPU_PRINCIPLED_CLEARCOAT];
	p.clearcoat_gloss = m.principled[PRGPU_PRINCIPLED_CLEARCOAT_GLOSS];
	return p;
}
// RoughConductorMaterial::eval (roughconductor.cpp:41-65), RoughDielectricMaterial::eval (roughdielectric.cpp:184-205).
// `delta`: MaterialSampleFlag::DeltaDistribution.  Out of line: only scenes with rough materials pay for it.
static __device__ PR_CLOSURE void PR_UV(rough_eval)(const DevScene& s, const prgpu_material& mat, const Blob& wl, const Blob& cie_y, V3 Vt, V3 Lt, Blob& weight, Blob& pdf, bool& delta PR_UV_PARAM)
{
	if (mat.kind == PRGPU_MAT_PRINCIPLED) { // PrincipledMaterial::eval (principled.cpp:499-528)
		const Principled c = PR_UV(principled_closure)(s, mat, wl, cie_y PR_UV_ARG);
		delta			   = c.is_delta();
		if (delta) {
			weight = blob(0);
			pdf	   = blob(0);
			return;
		}
		principled_eval_pdf(c, Vt, Lt, weight, pdf);
		return;
	}
	const RoughDistribution d = rough_distribution(mat);
	delta					  = d.is_delta();
	if (delta) {
		weight = blob(0);
		pdf	   = blob(0);
		return;
	}
	if (mat.kind == PRGPU_MAT_ROUGH_CONDUCTOR) {
		const Blob eta = PR_UV(spectrum_eval_cold)(s, mat.ior, wl PR_UV_ARG), kk = PR_UV(spectrum_eval_cold)(s, mat.k, wl PR_UV_ARG);
		Blob factor;
		for (int i = 0; i < 4; ++i)
			factor.v[i] = mf_reflection_eval(d, Lt, Vt, true, eta.v[i], kk.v[i]);
		weight = PR_UV(spectrum_eval_cold)(s, mat.albedo, wl PR_UV_ARG) * factor;
		pdf	   = blob(mf_reflection_pdf(d, Lt, Vt));
	} else {
		const Blob spec	 = PR_UV(spectrum_eval_cold)(s, mat.albedo, wl PR_UV_ARG);
		const Blob trans = mat.transmission != INVALID ? PR_UV(spectrum_eval_cold)(s, mat.transmission, wl PR_UV_ARG) : spec;
		const Blob ior	 = PR_UV(spectrum_eval_cold)(s, mat.ior, wl PR_UV_ARG);
		weight			 = rough_dielectric_eval(d, Vt, Lt, spec, trans, ior);
		pdf				 = rough_dielectric_pdf(d, Vt, Lt, ior);
	}
}
// RoughConductorMaterial::sample (roughconductor.cpp:83-117), RoughDielectricMaterial::sample (roughdielectric.cpp:222-254)
static __device__ PR_CLOSURE void PR_UV(rough_sample)(const DevScene& s, const prgpu_material& mat, const Blob& wl, const Blob& cie_y, V3 Vt, uint64_t& rnd, V3& Lt, Blob& integral_weight, Blob& pdf_s,
										  bool& delta, bool& hero_collapsing PR_UV_PARAM)
{
	if (mat.kind == PRGPU_MAT_PRINCIPLED) { // PrincipledMaterial::sample (principled.cpp:548-590)
		const Principled c = PR_UV(principled_closure)(s, mat, wl, cie_y PR_UV_ARG);
		Lt				   = principled_sample(c, rnd, Vt);
		delta			   = c.is_delta();
		hero_collapsing	   = false; // the material sets no SpectralVarying flag
		if (v3_is_zero(Lt, 1e-5f)) {
			Lt				= v3(0, 0, 0);
			integral_weight = blob(0);
			pdf_s			= blob(0);
			return;
		}
		principled_eval_pdf(c, Vt, Lt, integral_weight, pdf_s);
		if (pdf_s.v[0] > PR_EPS)
			integral_weight = integral_weight / pdf_s.v[0];
		if (delta)
			pdf_s = blob(1);
		return;
	}
	const RoughDistribution d = rough_distribution(mat);
	delta					  = d.is_delta();
	if (mat.kind == PRGPU_MAT_ROUGH_CONDUCTOR) {
		const float u0 = rng_float(rnd), u1 = rng_float(rnd);
		Lt				= mf_reflection_sample(d, u0, u1, Vt);
		hero_collapsing = delta && (spectrum_varying<PR_CLOSURES_IMG != 0>(s.spectra[mat.ior]) || spectrum_varying<PR_CLOSURES_IMG != 0>(s.spectra[mat.k]));
		if (!sv_same_hemisphere(Vt, Lt)) { // MaterialSampleOutput::Reject
			Lt				= v3(0, 0, 0);
			integral_weight = blob(0);
			pdf_s			= blob(0);
			return;
		}
		const Blob eta = PR_UV(spectrum_eval_cold)(s, mat.ior, wl PR_UV_ARG), kk = PR_UV(spectrum_eval_cold)(s, mat.k, wl PR_UV_ARG);
		Blob factor;
		for (int i = 0; i < 4; ++i)
			factor.v[i] = mf_reflection_eval(d, Lt, Vt, true, eta.v[i], kk.v[i]);
		integral_weight = PR_UV(spectrum_eval_cold)(s, mat.albedo, wl PR_UV_ARG) * factor;
		pdf_s			= blob(mf_reflection_pdf(d, Lt, Vt));
	} else {
		const Blob spec	 = PR_UV(spectrum_eval_cold)(s, mat.albedo, wl PR_UV_ARG);
		const Blob trans = mat.transmission != INVALID ? PR_UV(spectrum_eval_cold)(s, mat.transmission, wl PR_UV_ARG) : spec;
		const Blob ior	 = PR_UV(spectrum_eval_cold)(s, mat.ior, wl PR_UV_ARG);
		hero_collapsing	 = delta && spectrum_varying<PR_CLOSURES_IMG != 0>(s.spectra[mat.ior]);
		// RoughDielectricClosure::sample (roughdielectric.cpp:124-137): branch on the hero wavelength's Fresnel term
		const float F  = fresnel_dielectric(Vt.z, DIELECTRIC_AIR, ior.v[0]);
		const float ub = rng_float(rnd);
		const float u0 = rng_float(rnd), u1 = rng_float(rnd);
		Lt = ub <= F ? mf_reflection_sample(d, u0, u1, Vt) : mf_transmission_sample(d, u0, u1, Vt, DIELECTRIC_AIR, ior.v[0]);
		if (v3_is_zero(Lt, 1e-5f)) { // Eigen isZero() with the default precision
			Lt				= v3(0, 0, 0);
			integral_weight = blob(0);
			pdf_s			= blob(0);
			return;
		}
		integral_weight = rough_dielectric_eval(d, Vt, Lt, spec, trans, ior);
		pdf_s			= rough_dielectric_pdf(d, Vt, Lt, ior);
	}
	if (pdf_s.v[0] > PR_EPS)
		integral_weight = integral_weight / pdf_s.v[0];
	if (delta)
		pdf_s = blob(1);
}

#undef PR_UV
#undef PR_UV_PARAM
#undef PR_UV_ARG
