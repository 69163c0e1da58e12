// mini_json.hpp — the subset of JSON the voxelPS config files use (one flat object of string / number / bool values,
// config/*.json).  Replaces nlohmann::json in ConfigLoader.h:16-170 (not available in this build environment).
// JsonNode, below, reads a whole value with nested objects and arrays: the light file of `voxelPS --relight`.
#pragma once
#include <cctype>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace psgsdf_host {

struct JsonValue {
    enum Kind { STRING, NUMBER, BOOL, NUL } kind = NUL;
    std::string s; double n = 0; bool b = false;
};

class JsonObject {
    std::map<std::string, JsonValue> kv_;
    std::vector<std::string> order_;
    static void skip(const std::string& t, size_t& i) { while (i < t.size() && std::isspace((unsigned char)t[i])) ++i; }
    static bool parse_string(const std::string& t, size_t& i, std::string& out) {
        if (i >= t.size() || t[i] != '"') return false;
        ++i; out.clear();
        while (i < t.size() && t[i] != '"') {
            if (t[i] == '\\' && i + 1 < t.size()) { char c = t[++i]; out += c == 'n' ? '\n' : c == 't' ? '\t' : c; }
            else out += t[i];
            ++i;
        }
        if (i >= t.size()) return false;
        ++i; return true;
    }
public:
    bool parse(const std::string& text) {
        size_t i = 0; skip(text, i);
        if (i >= text.size() || text[i] != '{') return false;
        ++i;
        while (true) {
            skip(text, i);
            if (i < text.size() && text[i] == '}') return true;
            std::string key; if (!parse_string(text, i, key)) return false;
            skip(text, i); if (i >= text.size() || text[i] != ':') return false; ++i; skip(text, i);
            JsonValue v;
            if (text[i] == '"') { v.kind = JsonValue::STRING; if (!parse_string(text, i, v.s)) return false; }
            else if (!text.compare(i, 4, "true")) { v.kind = JsonValue::BOOL; v.b = true; i += 4; }
            else if (!text.compare(i, 5, "false")) { v.kind = JsonValue::BOOL; v.b = false; i += 5; }
            else if (!text.compare(i, 4, "null")) { v.kind = JsonValue::NUL; i += 4; }
            else { char* end = nullptr; v.n = std::strtod(text.c_str() + i, &end); if (end == text.c_str() + i) return false; v.kind = JsonValue::NUMBER; i = end - text.c_str(); }
            if (!kv_.count(key)) order_.push_back(key);
            kv_[key] = v;
            skip(text, i);
            if (i < text.size() && text[i] == ',') { ++i; continue; }
            if (i < text.size() && text[i] == '}') return true;
            return false;
        }
    }
    bool load(const std::string& path) { std::ifstream f(path); if (!f.is_open()) return false; std::stringstream ss; ss << f.rdbuf(); return parse(ss.str()); }
    bool contains(const std::string& k) const { return kv_.count(k) != 0; }
    std::string str(const std::string& k) const { return kv_.at(k).s; }
    double num(const std::string& k) const { const JsonValue& v = kv_.at(k); return v.kind == JsonValue::BOOL ? (v.b ? 1.0 : 0.0) : v.n; }
    bool boolean(const std::string& k) const { const JsonValue& v = kv_.at(k); return v.kind == JsonValue::BOOL ? v.b : v.n != 0; }
    // `save_conf << std::setw(4) << config` (ConfigLoader.h:161-165): 4-space indented dump, keys sorted like nlohmann's std::map
    void dump(std::ostream& os) const {
        os << "{\n"; size_t k = 0;
        for (auto& kv : kv_) {
            os << "    \"" << kv.first << "\": ";
            const JsonValue& v = kv.second;
            if (v.kind == JsonValue::STRING) os << '"' << v.s << '"'; else if (v.kind == JsonValue::BOOL) os << (v.b ? "true" : "false"); else if (v.kind == JsonValue::NUL) os << "null"; else os << v.n;
            os << (++k < kv_.size() ? ",\n" : "\n");
        }
        os << "}";
    }
};

// A whole JSON value with nested objects and arrays (the light file of `voxelPS --relight`; the config files stay flat and go through JsonObject).
struct JsonNode {
    enum Kind { OBJECT, ARRAY, STRING, NUMBER, BOOL, NUL } kind = NUL;
    std::string s; double n = 0; bool b = false;
    std::vector<std::string> keys;      // OBJECT: the key of every item
    std::vector<JsonNode> items;        // OBJECT, ARRAY
    const JsonNode* get(const std::string& k) const { for (size_t i = 0; i < keys.size(); ++i) if (keys[i] == k) return &items[i]; return nullptr; }
    // the whole text is one value (true), or malformed (false)
    bool parse(const std::string& t) { size_t i = 0; if (!value(t, i, 0)) return false; ws(t, i); return i == t.size(); }
    bool load(const std::string& path) { std::ifstream f(path); if (!f.is_open()) return false; std::stringstream ss; ss << f.rdbuf(); return parse(ss.str()); }
private:
    static void ws(const std::string& t, size_t& i) { while (i < t.size() && std::isspace((unsigned char)t[i])) ++i; }
    static bool string(const std::string& t, size_t& i, std::string& out) {
        if (i >= t.size() || t[i] != '"') return false;
        ++i; out.clear();
        while (i < t.size() && t[i] != '"') {
            if (t[i] == '\\' && i + 1 < t.size()) { char c = t[++i]; out += c == 'n' ? '\n' : c == 't' ? '\t' : c; }
            else out += t[i];
            ++i;
        }
        if (i >= t.size()) return false;
        ++i; return true;
    }
    bool value(const std::string& t, size_t& i, int depth) {
        ws(t, i);
        if (i >= t.size() || depth > 32) return false;
        if (t[i] == '{' || t[i] == '[') {
            const bool obj = t[i] == '{'; const char close = obj ? '}' : ']';
            kind = obj ? OBJECT : ARRAY; ++i; ws(t, i);
            if (i < t.size() && t[i] == close) { ++i; return true; }
            while (true) {
                if (obj) { std::string k; ws(t, i); if (!string(t, i, k)) return false; ws(t, i); if (i >= t.size() || t[i] != ':') return false; ++i; keys.push_back(k); }
                items.emplace_back();
                if (!items.back().value(t, i, depth + 1)) return false;
                ws(t, i);
                if (i < t.size() && t[i] == ',') { ++i; continue; }
                if (i < t.size() && t[i] == close) { ++i; return true; }
                return false;
            }
        }
        if (t[i] == '"') { kind = STRING; return string(t, i, s); }
        if (!t.compare(i, 4, "true")) { kind = BOOL; b = true; i += 4; return true; }
        if (!t.compare(i, 5, "false")) { kind = BOOL; b = false; i += 5; return true; }
        if (!t.compare(i, 4, "null")) { kind = NUL; i += 4; return true; }
        char* end = nullptr; n = std::strtod(t.c_str() + i, &end);
        if (end == t.c_str() + i) return false;
        kind = NUMBER; i = end - t.c_str(); return true;
    }
};

}  // namespace psgsdf_host
