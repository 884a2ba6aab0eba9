// glyph_rule_check.cpp -- csrc/smh_glyph_rule.h as a stand-alone host program (tests/test_label_text_host.py compiles it with the host
// compiler, with -fsanitize=address,undefined where that links): reads frames from a file, runs the header's host path over them
// (glyph_template_fault, glyph_atlas_fill, frame_read) and writes one smhv_label_text_frame per frame.
//   glyph_rule_check <in> <out>
// in:  u32 frames; per frame: u32 n_templates, accept_num, accept_den, reserved; n_templates smhv_glyph_template;
//      one smhv_scale_label_frame; SMHV_LABEL_FRAME_CROP_BYTES cell bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "smh_glyph_rule.h"

static bool get(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
	if (argc != 3) { fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
	uint32_t frames = 0;
	if (!get(in, &frames, 4)) return 3;
	std::vector<uint8_t> cells(SMHV_LABEL_FRAME_CROP_BYTES);
	for (uint32_t i = 0; i < frames; ++i) {
		uint32_t head[4];
		if (!get(in, head, sizeof head) || head[0] == 0 || head[0] > SMHV_ATLAS_MAX_TEMPLATES) { fprintf(stderr, "frame %u: bad head\n", i); return 3; }
		std::vector<smhv_glyph_template> t(head[0]);
		smhv_scale_label_frame f;
		if (!get(in, t.data(), sizeof(smhv_glyph_template) * t.size()) || !get(in, &f, sizeof f) || !get(in, cells.data(), cells.size())) return 3;
		for (uint32_t k = 0; k < head[0]; ++k)
			if (const char *why = smh::glyph_template_fault(&t[k])) { fprintf(stderr, "frame %u: template %u: %s\n", i, k, why); return 4; }
		smh::GlyphAtlas A;
		smh::glyph_atlas_fill(&A, t.data(), head[0], head[1], head[2]);
		smhv_label_text_frame rec;
		smh::frame_read(&A, &f, cells.data(), &rec);
		if (fwrite(&rec, 1, sizeof rec, out) != sizeof rec) return 5;
	}
	fclose(in);
	if (fclose(out) != 0) return 5;
	printf("ok: %u frames\n", frames);
	return 0;
}
