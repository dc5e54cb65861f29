// bgs_describe.inc — one description of a class's ./config/<Class>.xml serves both directions.  A class names each key once, in the
// reference's order, with the member it lives in and its default: describe(io) { io("threshold", threshold, 15); ... }.  Loading
// reads every key (a missing file or key gives the default, like cvRead*ByName on a NULL storage); saving writes them in the same
// order.  The overload is picked by the member's type, so the default keeps its own literal type up to the call (0.333f and 0.333
// widen to different doubles).  Written against XmlConfig alone; include inside the namespace, right after it.
class XmlIo {
 public:
  XmlIo(XmlConfig& fs, bool load) : fs_(fs), load_(load) {}
  void operator()(const char* key, int& v, int def) {
    if (load_) v = fs_.readInt(key, def); else fs_.writeInt(key, v);
  }
  void operator()(const char* key, bool& v, int def) {  // the reference keeps its flags in cvReadIntByName / cvWriteInt
    if (load_) v = fs_.readInt(key, def) != 0; else fs_.writeInt(key, v);
  }
  void operator()(const char* key, double& v, double def) {
    if (load_) v = fs_.readReal(key, def); else fs_.writeReal(key, v);
  }
  void operator()(const char* key, float& v, double def) {  // narrowed on the way in, written as the double the float widens to
    if (load_) v = (float)fs_.readReal(key, def); else fs_.writeReal(key, v);
  }
  void asInt(const char* key, double& v, int def) {  // an int in the XML, a double in the class (DPMeanBGS, DPAdaptiveMedianBGS)
    if (load_) v = fs_.readInt(key, def); else fs_.writeInt(key, (int)v);
  }
#ifdef BGS_HIP_XML_HAS_STRINGS
  void operator()(const char* key, std::string& v, const char* def) {
    if (load_) v = fs_.readString(key, def); else fs_.writeString(key, v);
  }
#endif

 private:
  XmlConfig& fs_;
  bool load_;
};

// What saveConfig() and loadConfig() of every class are.  loaded() runs after every load: where a class hands values on.
class XmlDescribed {
 protected:
  virtual ~XmlDescribed() {}
  virtual void describe(XmlIo& io) = 0;
  virtual void loaded() {}
  void saveDescribed(const std::string& path) {
    XmlConfig fs;
    fs.beginWrite();
    XmlIo io(fs, false);
    describe(io);
    fs.save(path);
  }
  void loadDescribed(const std::string& path) {
    XmlConfig fs;
    fs.load(path);
    XmlIo io(fs, true);
    describe(io);
    loaded();
  }
};
