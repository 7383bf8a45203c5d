// obj_parser.cpp — restatement of raytrace_lib/src/obj_parser.rs:20-73.
// "v x y z" and "f a[/..] b c ..." lines only, 1-based indices, first three
// corners of a face; everything else is ignored.  Where the reference panics
// (unwrap / assert / index out of bounds) this throws std::runtime_error.
//
// ObjMode::Robust is an opt-in EXTENSION the reference does not have (its
// parser would panic or silently drop geometry on such files): faces with more
// than three corners are fan-triangulated (c0, c_i, c_i+1), negative indices
// count back from the vertices read so far (OBJ convention), comment and blank
// lines inside face data are tolerated, degenerate triangles are skipped
// instead of aborting the load.  The default stays the reference's behaviour.
#include <cerrno>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "raytrace.hpp"

namespace raytrace {
namespace obj_parser {

namespace {
// str::split_whitespace
std::vector<std::string> fields(const std::string& s) {
    std::vector<std::string> out;
    size_t i = 0;
    while (i < s.size()) {
        while (i < s.size() && isspace((unsigned char)s[i])) i++;
        size_t j = i;
        while (j < s.size() && !isspace((unsigned char)s[j])) j++;
        if (j > i) out.push_back(s.substr(i, j - i));
        i = j;
    }
    return out;
}
float parse_f32(const std::string& tok, const std::string& line) {
    char* end = nullptr;
    errno = 0;
    const float x = strtof(tok.c_str(), &end);  // correctly rounded decimal -> f32, like Rust's parse::<f32>
    if (end == tok.c_str() || *end != '\0') throw std::runtime_error("parse_obj: bad number in vertex line: " + line);
    return x;
}
size_t parse_index(const std::string& tok, const std::string& line) {
    const std::string head = tok.substr(0, tok.find('/'));  // x.split('/').nth(0)
    if (head.empty() || head.find_first_not_of("0123456789") != std::string::npos)
        throw std::runtime_error("parse_obj: bad index in face line: " + line);
    return (size_t)strtoull(head.c_str(), nullptr, 10);
}
// Robust mode: "-k" is the k-th last vertex read so far; returns a 1-based absolute index (0 = invalid)
size_t parse_index_relative(const std::string& tok, const std::string& line, size_t nverts) {
    const std::string head = tok.substr(0, tok.find('/'));
    if (head.size() > 1 && head[0] == '-' && head.find_first_not_of("0123456789", 1) == std::string::npos) {
        const size_t back = (size_t)strtoull(head.c_str() + 1, nullptr, 10);
        return back >= 1 && back <= nverts ? nverts - back + 1 : 0;
    }
    return parse_index(tok, line);
}
// normals9: the third field of a face corner "a/b/c" or "a//c" as a 1-based index into the vn lines (Robust: "-k" counts back from
// the normals read so far); 0 = none or invalid
size_t parse_normal_index(const std::string& tok, size_t nnormals, bool robust) {
    const size_t s1 = tok.find('/');
    const size_t s2 = s1 == std::string::npos ? s1 : tok.find('/', s1 + 1);
    if (s2 == std::string::npos) return 0;
    const std::string f = tok.substr(s2 + 1);
    if (robust && f.size() > 1 && f[0] == '-' && f.find_first_not_of("0123456789", 1) == std::string::npos) {
        const size_t back = (size_t)strtoull(f.c_str() + 1, nullptr, 10);
        return back >= 1 && back <= nnormals ? nnormals - back + 1 : 0;
    }
    if (f.empty() || f.find_first_not_of("0123456789") != std::string::npos) return 0;
    return (size_t)strtoull(f.c_str(), nullptr, 10);
}
// uvs6: the second field of a face corner "a/b" or "a/b/c" as a 1-based index into the vt lines (Robust: "-k" counts back from the
// ones read so far); 0 = none or invalid
size_t parse_uv_index(const std::string& tok, size_t nuvs, bool robust) {
    const size_t s1 = tok.find('/');
    if (s1 == std::string::npos) return 0;
    const size_t s2 = tok.find('/', s1 + 1);
    const std::string f = tok.substr(s1 + 1, s2 == std::string::npos ? std::string::npos : s2 - s1 - 1);
    if (robust && f.size() > 1 && f[0] == '-' && f.find_first_not_of("0123456789", 1) == std::string::npos) {
        const size_t back = (size_t)strtoull(f.c_str() + 1, nullptr, 10);
        return back >= 1 && back <= nuvs ? nuvs - back + 1 : 0;
    }
    if (f.empty() || f.find_first_not_of("0123456789") != std::string::npos) return 0;
    return (size_t)strtoull(f.c_str(), nullptr, 10);
}
}  // namespace

std::vector<Triangle> parse_obj(const std::string& path, const Vec3& offset, float scale,
                                const std::tuple<Vec3, Vec3, Vec3>& transform, const SurfaceKind& surface,
                                float edge_thickness, ObjMode mode, std::vector<float>* normals9, std::vector<float>* uvs6) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("parse_obj: cannot read " + path);
    std::vector<Vec3> vertices;
    std::vector<std::vector<size_t>> faces;
    std::vector<Vec3> vnormals;                 // normals9 only
    std::vector<std::vector<size_t>> fnormals;  // normals9 only: per face, the corners' normal indices
    std::vector<std::pair<float, float>> vuvs;  // uvs6 only
    std::vector<std::vector<size_t>> fuvs;      // uvs6 only: per face, the corners' uv indices
    std::string line;
    while (std::getline(f, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.compare(0, 2, "v ") == 0) {
            const auto parts = fields(line.substr(2));
            if (parts.size() != 3) throw std::runtime_error("parse_obj: vertex line needs exactly 3 numbers: " + line);
            vertices.push_back(make_vec(parse_f32(parts[0], line), parse_f32(parts[1], line), parse_f32(parts[2], line)));
        } else if (line.compare(0, 2, "f ") == 0) {
            std::vector<size_t> corners;
            for (const auto& tok : fields(line.substr(2)))
                corners.push_back(mode == ObjMode::Robust ? parse_index_relative(tok, line, vertices.size()) : parse_index(tok, line));
            faces.push_back(std::move(corners));
            if (normals9) {
                std::vector<size_t> ni;
                for (const auto& tok : fields(line.substr(2))) ni.push_back(parse_normal_index(tok, vnormals.size(), mode == ObjMode::Robust));
                fnormals.push_back(std::move(ni));
            }
            if (uvs6) {
                std::vector<size_t> ui;
                for (const auto& tok : fields(line.substr(2))) ui.push_back(parse_uv_index(tok, vuvs.size(), mode == ObjMode::Robust));
                fuvs.push_back(std::move(ui));
            }
        } else if (uvs6 && line.compare(0, 3, "vt ") == 0) {
            const auto parts = fields(line.substr(3));
            if (parts.size() < 2 || parts.size() > 3) throw std::runtime_error("parse_obj: texture coordinate line needs 2 or 3 numbers: " + line);
            vuvs.emplace_back(parse_f32(parts[0], line), parse_f32(parts[1], line));
        } else if (normals9 && line.compare(0, 3, "vn ") == 0) {
            const auto parts = fields(line.substr(3));
            if (parts.size() != 3) throw std::runtime_error("parse_obj: normal line needs exactly 3 numbers: " + line);
            vnormals.push_back(make_vec(parse_f32(parts[0], line), parse_f32(parts[1], line), parse_f32(parts[2], line)));
        }
    }
    std::vector<Triangle> objs;
    objs.reserve(faces.size());
    auto place = [&](size_t idx) {  // obj_parser.rs:61-70
        if (idx < 1 || idx > vertices.size()) throw std::runtime_error("parse_obj: face index out of range");
        return vertices[idx - 1].mult(scale).change_basis(transform).add(offset);
    };
    auto push_normals = [&](size_t fi, size_t a, size_t b, size_t c) {  // of the triangle just pushed: corners a, b, c of face fi
        if (!normals9) return;
        for (size_t k : {a, b, c}) {
            const size_t idx = fnormals[fi][k];
            if (idx < 1 || idx > vnormals.size()) throw std::runtime_error("parse_obj: a face corner has no normal index, or one out of range");
            const Vec3 n = vnormals[idx - 1].change_basis(transform).unit();
            normals9->insert(normals9->end(), n.v, n.v + 3);
        }
    };
    auto push_uvs = [&](size_t fi, size_t a, size_t b, size_t c) {  // of the triangle just pushed, likewise
        if (!uvs6) return;
        for (size_t k : {a, b, c}) {
            const size_t idx = fuvs[fi][k];
            if (idx < 1 || idx > vuvs.size()) throw std::runtime_error("parse_obj: a face corner has no texture coordinate index, or one out of range");
            uvs6->push_back(vuvs[idx - 1].first);
            uvs6->push_back(vuvs[idx - 1].second);
        }
    };
    for (size_t fi = 0; fi < faces.size(); fi++) {
        const auto& face = faces[fi];
        if (face.size() < 3) throw std::runtime_error("parse_obj: face with fewer than 3 corners");
        if (mode == ObjMode::Reference) {  // first three corners, whatever follows (obj_parser.rs:63-65)
            Vec3 pts[3] = {place(face[0]), place(face[1]), place(face[2])};
            objs.push_back(make_triangle(pts, surface, edge_thickness));
            push_normals(fi, 0, 1, 2);
            push_uvs(fi, 0, 1, 2);
            continue;
        }
        for (size_t k = 1; k + 1 < face.size(); k++) {  // fan: (c0, ck, ck+1)
            Vec3 pts[3] = {place(face[0]), place(face[k]), place(face[k + 1])};
            try { objs.push_back(make_triangle(pts, surface, edge_thickness)); }
            catch (const std::runtime_error&) { continue; }  // degenerate sliver of a polygon: skipped (the reference would panic, raytrace.rs:357)
            push_normals(fi, 0, k, k + 1);
            push_uvs(fi, 0, k, k + 1);
        }
    }
    return objs;
}

}  // namespace obj_parser
}  // namespace raytrace
