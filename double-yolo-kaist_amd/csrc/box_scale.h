// The un-letterbox transform of one box, shared by dyk_scale_coords (boxes.hip) and dyk_eval_match (evalmap.hip): one
// definition, so the evaluator's boxes are bit for bit those of scale_coords.  Plain fp32, no contraction: every value
// rounds like the torch-CPU expression of the reference, (x - pad) / gain -> clamp (build_utils/utils.py:60-92).
#pragma once
#pragma clang fp contract(off)

__device__ inline float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // NaN passes through like torch.clamp_

__device__ inline void unletterbox(float& x1, float& y1, float& x2, float& y2, float pad_x, float pad_y, float gain) {
    x1 = (x1 - pad_x) / gain; x2 = (x2 - pad_x) / gain;
    y1 = (y1 - pad_y) / gain; y2 = (y2 - pad_y) / gain;
}

__device__ inline void clip_box(float& x1, float& y1, float& x2, float& y2, float w0, float h0) {
    x1 = clampf(x1, 0.f, w0); y1 = clampf(y1, 0.f, h0);
    x2 = clampf(x2, 0.f, w0); y2 = clampf(y2, 0.f, h0);
}
